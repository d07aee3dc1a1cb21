// gsrt_image_loss.hip -- the photometric loss of a frame on the device (gsrt_image_loss): L1 + D-SSIM against a target
// image, the four scalars {loss, l1, ssim, mse} and the gradient with respect to the frame in the framebuffer's own
// [H][W][4] layout. The formulas are gsrt.h's.
//
// Three kernels on the render stream, at ordinary priority:
//   k_loss_stats    per tile of 32 x 16 pixels (512 lanes, one pixel a lane): x and y of the tile plus a 5-pixel halo
//                   (42 x 26 pixels, zeros outside the image) go to LDS, all three channels from one 16-byte read per
//                   pixel. Per channel the five window sums (x, y, x^2, y^2, xy) are formed separably, rows first
//                   (26 x 32 row sums into LDS), then columns (11 taps a lane). Each lane forms its pixel's SSIM term
//                   and, for a call with a gradient, the three derivative maps, which go to the workspace as nine
//                   planes of H x W floats. The tile's sums of |x - y|, (x - y)^2 and the SSIM term are reduced in
//                   double (wave shuffles, then LDS in wave order) and stored as the tile's three partial sums.
//   k_loss_scalars  one workgroup: lane t adds the partial sums of tiles t, t + 256, ... in that order, the 256 lane sums
//                   are added by a fixed tree in LDS, and lane 0 forms the four scalars in double and rounds each once.
//   k_loss_grad     the same tiling: a channel's three derivative maps plus halo (zeros outside the image) go to LDS, are
//                   convolved separably, and each lane combines its three sums with its x, y and sign(x - y) and stores
//                   one 16-byte pixel {g_r, g_g, g_b, +0}. A gather: no pixel is written by two lanes.
// No atomics anywhere: every output word is a fixed expression of the inputs, so two runs give the same bits.
//
// LDS banks. Rows pass: a 32-lane half wave takes 32 consecutive columns of one halo row, so every tap reads 32
// consecutive words. Columns pass: a half wave is one row of the tile and reads 32 consecutive words of a row of row
// sums (leading dimension 32). Neither has a bank conflict; the halo tiles need no padding.
// Occupancy (workgroups of 8 waves, two per SIMD). k_loss_stats: 2 x 3 x 1092 + 5 x 832 floats + 24 doubles = 43,040 B
// of LDS, so three workgroups (24 waves) per CU; 44 VGPRs with the gradient, 70 without, neither the limit.
// k_loss_grad: 3 x 1092 + 3 x 832 floats = 23,088 B of LDS would admit four workgroups, its 91 VGPRs admit five waves
// per SIMD, which is two whole workgroups (16 waves) per CU. Neither kernel spills.
//
// gsrt_frame_loss (the second half of the file): the same three kernels with a background, a pixel mask and a depth term,
// as kernels of their own (k_frame_stats, k_frame_scalars, k_frame_grad), so that the ones above stay as they are.
//   k_frame_stats   composites and masks every halo pixel with its own alpha and mask while filling the same LDS tiles, so
//                   the window sums see x' = m (C + (1 - a) bg), y' = m y; each lane then adds its own pixel's depth term
//                   m |D / a - t| and sample count: five partial sums a tile.
//   k_frame_scalars five sums in, six scalars out, the same lane assignment and tree.
//   k_frame_grad    the same convolution, then {m g_r, m g_g, m g_b, alpha slot} and the grad_depth word, still a gather.
// The LDS arrays, the lane-to-word maps and so the bank argument above are unchanged. Occupancy: k_frame_stats 43,168 B
// of LDS (two more rows of 8 doubles), three workgroups per CU as before; 46 VGPRs with the gradient, 72 without.
// k_frame_grad 23,088 B of LDS and 60 VGPRs: eight waves per SIMD, four workgroups (32 waves, the cap) per CU.
// k_frame_scalars 24 VGPRs, 10,240 B. No kernel uses scratch.
#include <cstdint>

#include "gsrt_internal.hpp"

namespace gsrt {

constexpr int kLossTileW = 32, kLossTileH = 16;  // one pixel a lane
constexpr int kLossBlock = kLossTileW * kLossTileH;
constexpr int kLossR = 5;                        // the window reaches 5 pixels each way
constexpr int kLossHaloW = kLossTileW + 2 * kLossR, kLossHaloH = kLossTileH + 2 * kLossR;
constexpr int kLossHalo = kLossHaloW * kLossHaloH;  // 1092 pixels
constexpr int kLossRows = kLossHaloH * kLossTileW;  // 832 row sums per quantity
constexpr float kLossC1 = 0.01f * 0.01f, kLossC2 = 0.03f * 0.03f;

// exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0..10, normalised to sum 1 in double, each rounded to float once
#define GSRT_LOSS_WINDOW                                                                                              \
    {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f, 0x1.b43c4p-3f, \
     0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}
__constant__ float c_loss_window[11] = GSRT_LOSS_WINDOW;
static const float h_loss_window[11] = GSRT_LOSS_WINDOW;

void image_loss_window(float out[11]) {
    for (int i = 0; i < 11; ++i) out[i] = h_loss_window[i];
}

uint32_t image_loss_tiles(uint32_t width, uint32_t height) {
    return ((width + kLossTileW - 1) / kLossTileW) * ((height + kLossTileH - 1) / kLossTileH);
}

// the sum of v over the workgroup's 512 lanes in double, in a fixed order: down each wave by shuffles, then the eight
// wave sums in wave order. Valid in lane 0. red: 8 doubles of LDS, free to reuse after the next barrier.
__device__ inline double loss_block_sum(double v, double* red) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const uint32_t t = threadIdx.x;
    if ((t & 63u) == 0) red[t >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (t == 0)
        for (int w = 0; w < kLossBlock / 64; ++w) s += red[w];
    return s;
}

template <bool kGrad, int kTargetChannels>
__global__ __launch_bounds__(kLossBlock) void k_loss_stats(uint32_t W, uint32_t H, const float* __restrict__ rgba,
                                                           const float* __restrict__ target, float* __restrict__ maps,
                                                           double* __restrict__ partial) {
    __shared__ float sx[3][kLossHalo], sy[3][kLossHalo];
    __shared__ float rows[5][kLossRows];
    __shared__ double red[3][kLossBlock / 64];
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * kLossTileW, y0 = blockIdx.y * kLossTileH;

    for (int i = t; i < kLossHalo; i += kLossBlock) {
        const int hy = i / kLossHaloW, hx = i - hy * kLossHaloW;
        const int px = x0 + hx - kLossR, py = y0 + hy - kLossR;
        float a[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
        if (px >= 0 && py >= 0 && px < (int)W && py < (int)H) {
            const size_t p = (size_t)py * W + px;
            const float4 v = reinterpret_cast<const float4*>(rgba)[p];
            a[0] = v.x, a[1] = v.y, a[2] = v.z;
            if (kTargetChannels == 4) {
                const float4 u = reinterpret_cast<const float4*>(target)[p];
                b[0] = u.x, b[1] = u.y, b[2] = u.z;
            } else {
                b[0] = target[3 * p], b[1] = target[3 * p + 1], b[2] = target[3 * p + 2];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) sx[c][i] = a[c], sy[c][i] = b[c];
    }
    __syncthreads();

    float w[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) w[k] = c_loss_window[k];

    const int tx = t & (kLossTileW - 1), ty = t / kLossTileW;
    const int px = x0 + tx, py = y0 + ty;
    const bool inside = px < (int)W && py < (int)H;
    const size_t plane = (size_t)W * H, pix = (size_t)py * W + px;
    double sum_abs = 0.0, sum_sq = 0.0, sum_map = 0.0;

    for (int c = 0; c < 3; ++c) {
        // rows: row sum (hy, cx) of the five quantities over halo columns cx .. cx + 10
        for (int i = t; i < kLossRows; i += kLossBlock) {
            const int hy = i / kLossTileW, cx = i - hy * kLossTileW;
            const float* ax = &sx[c][hy * kLossHaloW + cx];
            const float* ay = &sy[c][hy * kLossHaloW + cx];
            float m1 = 0.0f, m2 = 0.0f, e11 = 0.0f, e22 = 0.0f, e12 = 0.0f;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float a = ax[k], b = ay[k];
                m1 = fmaf(w[k], a, m1);
                m2 = fmaf(w[k], b, m2);
                e11 = fmaf(w[k], a * a, e11);
                e22 = fmaf(w[k], b * b, e22);
                e12 = fmaf(w[k], a * b, e12);
            }
            rows[0][i] = m1, rows[1][i] = m2, rows[2][i] = e11, rows[3][i] = e22, rows[4][i] = e12;
        }
        __syncthreads();
        // columns: the pixel's window sums over halo rows ty .. ty + 10
        float q[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 11; ++k)
#pragma unroll
            for (int j = 0; j < 5; ++j) q[j] = fmaf(w[k], rows[j][(ty + k) * kLossTileW + tx], q[j]);
        if (inside) {
            const float mu1 = q[0], mu2 = q[1];
            const float mu1mu1 = mu1 * mu1, mu2mu2 = mu2 * mu2, mu1mu2 = mu1 * mu2;
            const float s1 = q[2] - mu1mu1, s2 = q[3] - mu2mu2, s12 = q[4] - mu1mu2;
            const float A1 = 2.0f * mu1mu2 + kLossC1, A2 = 2.0f * s12 + kLossC2;
            const float B1 = (mu1mu1 + mu2mu2) + kLossC1, B2 = (s1 + s2) + kLossC2;
            const float den = B1 * B2;
            const float map = (A1 * A2) / den;
            const int centre = (ty + kLossR) * kLossHaloW + tx + kLossR;
            const float d = sx[c][centre] - sy[c][centre];
            sum_abs += (double)fabsf(d);
            sum_sq += (double)(d * d);
            sum_map += (double)map;
            if (kGrad) {
                // d map / d mu1 with the variances as functions of mu1 (sigma1^2 = E[x^2] - mu1^2, sigma12 = E[xy] -
                // mu1 mu2), d map / d sigma1^2 and d map / d sigma12
                const float d_mu = 2.0f * ((mu2 * (A2 - A1)) / den - (map * (mu1 * (B2 - B1))) / den);
                const float d_s1 = -(map / B2);
                const float d_s12 = (2.0f * A1) / den;
                maps[(size_t)(3 * c + 0) * plane + pix] = d_mu;
                maps[(size_t)(3 * c + 1) * plane + pix] = d_s1;
                maps[(size_t)(3 * c + 2) * plane + pix] = d_s12;
            }
        }
        __syncthreads();  // the row sums are overwritten by the next channel
    }

    // the three sums one after the other, each with its own LDS words
    const double s_abs = loss_block_sum(sum_abs, red[0]);
    const double s_sq = loss_block_sum(sum_sq, red[1]);
    const double s_map = loss_block_sum(sum_map, red[2]);
    if (t == 0) {
        double* o = partial + 3 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = s_abs, o[1] = s_sq, o[2] = s_map;
    }
}

// out = {loss, l1, ssim, mse} from the tiles' partial sums, in double, each rounded to float once
__global__ __launch_bounds__(256) void k_loss_scalars(uint32_t tiles, double count, float lambda,
                                                      const double* __restrict__ partial, float* __restrict__ out) {
    __shared__ double part[3][256];
    const uint32_t t = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    for (uint32_t b = t; b < tiles; b += 256)
        for (int j = 0; j < 3; ++j) s[j] += partial[3 * (size_t)b + j];
    for (int j = 0; j < 3; ++j) part[j][t] = s[j];
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (t < off)
            for (int j = 0; j < 3; ++j) part[j][t] += part[j][t + off];
        __syncthreads();
    }
    if (t == 0) {
        const double l1 = part[0][0] / count, mse = part[1][0] / count, ssim = part[2][0] / count;
        const double lam = (double)lambda;
        out[0] = (float)((1.0 - lam) * l1 + lam * (1.0 - ssim));
        out[1] = (float)l1;
        out[2] = (float)ssim;
        out[3] = (float)mse;
    }
}

// grad[p] = scale_l1 sign(x - y) - scale_ssim (conv(d_mu) + 2 x conv(d_s1) + y conv(d_s12)), alpha +0
template <int kTargetChannels>
__global__ __launch_bounds__(kLossBlock) void k_loss_grad(uint32_t W, uint32_t H, const float* __restrict__ rgba,
                                                          const float* __restrict__ target,
                                                          const float* __restrict__ maps, float scale_l1,
                                                          float scale_ssim, float* __restrict__ grad) {
    __shared__ float sm[3][kLossHalo];
    __shared__ float rows[3][kLossRows];
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * kLossTileW, y0 = blockIdx.y * kLossTileH;
    const int tx = t & (kLossTileW - 1), ty = t / kLossTileW;
    const int px = x0 + tx, py = y0 + ty;
    const bool inside = px < (int)W && py < (int)H;
    const size_t plane = (size_t)W * H, pix = (size_t)py * W + px;

    float w[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) w[k] = c_loss_window[k];

    float xv[3] = {0.0f, 0.0f, 0.0f}, yv[3] = {0.0f, 0.0f, 0.0f};
    if (inside) {
        const float4 v = reinterpret_cast<const float4*>(rgba)[pix];
        xv[0] = v.x, xv[1] = v.y, xv[2] = v.z;
        if (kTargetChannels == 4) {
            const float4 u = reinterpret_cast<const float4*>(target)[pix];
            yv[0] = u.x, yv[1] = u.y, yv[2] = u.z;
        } else {
            yv[0] = target[3 * pix], yv[1] = target[3 * pix + 1], yv[2] = target[3 * pix + 2];
        }
    }
    float g[3] = {0.0f, 0.0f, 0.0f};

    for (int c = 0; c < 3; ++c) {
        for (int i = t; i < kLossHalo; i += kLossBlock) {
            const int hy = i / kLossHaloW, hx = i - hy * kLossHaloW;
            const int qx = x0 + hx - kLossR, qy = y0 + hy - kLossR;
            const bool in = qx >= 0 && qy >= 0 && qx < (int)W && qy < (int)H;
            const size_t q = in ? (size_t)qy * W + qx : 0;
#pragma unroll
            for (int m = 0; m < 3; ++m) sm[m][i] = in ? maps[(size_t)(3 * c + m) * plane + q] : 0.0f;
        }
        __syncthreads();
        for (int i = t; i < kLossRows; i += kLossBlock) {
            const int hy = i / kLossTileW, cx = i - hy * kLossTileW;
            float r[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 11; ++k)
#pragma unroll
                for (int m = 0; m < 3; ++m) r[m] = fmaf(w[k], sm[m][hy * kLossHaloW + cx + k], r[m]);
#pragma unroll
            for (int m = 0; m < 3; ++m) rows[m][i] = r[m];
        }
        __syncthreads();
        float q[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 11; ++k)
#pragma unroll
            for (int m = 0; m < 3; ++m) q[m] = fmaf(w[k], rows[m][(ty + k) * kLossTileW + tx], q[m]);
        const float d = xv[c] - yv[c];
        const float sign = d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : d;  // sign(0) = 0; a NaN stays one
        const float gs = (q[0] + (2.0f * xv[c]) * q[1]) + yv[c] * q[2];
        g[c] = scale_l1 * sign - scale_ssim * gs;
        // the next channel's loads overwrite sm only after every lane has passed the barrier behind its row sums,
        // and rows only after the barrier behind its loads: nothing more is needed here
    }
    if (inside) reinterpret_cast<float4*>(grad)[pix] = make_float4(g[0], g[1], g[2], 0.0f);
}

void launch_image_loss(hipStream_t s, uint32_t width, uint32_t height, const float* rgba, const float* target,
                       uint32_t target_channels, float lambda, double* partial, float* maps, float* out, float* grad) {
    const dim3 grid((width + kLossTileW - 1) / kLossTileW, (height + kLossTileH - 1) / kLossTileH);
    const bool c4 = target_channels == 4;
    if (grad) {
        if (c4) hipLaunchKernelGGL((k_loss_stats<true, 4>), grid, dim3(kLossBlock), 0, s, width, height, rgba, target, maps, partial);
        else hipLaunchKernelGGL((k_loss_stats<true, 3>), grid, dim3(kLossBlock), 0, s, width, height, rgba, target, maps, partial);
    } else {
        if (c4) hipLaunchKernelGGL((k_loss_stats<false, 4>), grid, dim3(kLossBlock), 0, s, width, height, rgba, target, maps, partial);
        else hipLaunchKernelGGL((k_loss_stats<false, 3>), grid, dim3(kLossBlock), 0, s, width, height, rgba, target, maps, partial);
    }
    const double count = 3.0 * (double)width * (double)height;
    hipLaunchKernelGGL(k_loss_scalars, dim3(1), dim3(256), 0, s, grid.x * grid.y, count, lambda, partial, out);
    if (!grad) return;
    const float scale_l1 = (float)((1.0 - (double)lambda) / count), scale_ssim = (float)((double)lambda / count);
    if (c4) hipLaunchKernelGGL((k_loss_grad<4>), grid, dim3(kLossBlock), 0, s, width, height, rgba, target, maps, scale_l1, scale_ssim, grad);
    else hipLaunchKernelGGL((k_loss_grad<3>), grid, dim3(kLossBlock), 0, s, width, height, rgba, target, maps, scale_l1, scale_ssim, grad);
}

// ---- gsrt_frame_loss: the same three kernels with a background, a pixel mask and a depth term ----------------------
// Kernels of their own, so that gsrt_image_loss's stay the code objects they were. The options are uniform branches on
// the arguments (a NULL mask, a NULL depth, has_bg 0): a call with none of them executes the float32 operations of the
// kernels above in their order and gives their bits.

// x' and y' of pixel p: composited over the background, then masked (gsrt.h's order)
template <int kTargetChannels>
__device__ inline void frame_loss_pixel(const FrameLossArgs& A, size_t p, float x[3], float y[3]) {
    const float4 v = reinterpret_cast<const float4*>(A.rgba)[p];
    x[0] = v.x, x[1] = v.y, x[2] = v.z;
    if (kTargetChannels == 4) {
        const float4 u = reinterpret_cast<const float4*>(A.target)[p];
        y[0] = u.x, y[1] = u.y, y[2] = u.z;
    } else {
        y[0] = A.target[3 * p], y[1] = A.target[3 * p + 1], y[2] = A.target[3 * p + 2];
    }
    if (A.has_bg) {
        const float k = 1.0f - v.w;
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = x[c] + k * A.bg[c];
    }
    if (A.mask) {
        const float m = A.mask[p];
#pragma unroll
        for (int c = 0; c < 3; ++c) x[c] = m * x[c], y[c] = m * y[c];
    }
}

// a depth sample: a finite target depth above 0 under an alpha of at least alpha_min (a NaN of either is none)
__device__ inline bool frame_loss_sample(float a, float t, float alpha_min) {
    return t > 0.0f && t <= 3.402823466e+38f && a >= alpha_min;
}

template <bool kGrad, int kTargetChannels>
__global__ __launch_bounds__(kLossBlock) void k_frame_stats(const FrameLossArgs A, float* __restrict__ maps,
                                                            double* __restrict__ partial) {
    __shared__ float sx[3][kLossHalo], sy[3][kLossHalo];
    __shared__ float rows[5][kLossRows];
    __shared__ double red[5][kLossBlock / 64];
    const int t = threadIdx.x;
    const int W = (int)A.W, H = (int)A.H;
    const int x0 = blockIdx.x * kLossTileW, y0 = blockIdx.y * kLossTileH;

    // a halo pixel is composited and masked with its own alpha and mask
    for (int i = t; i < kLossHalo; i += kLossBlock) {
        const int hy = i / kLossHaloW, hx = i - hy * kLossHaloW;
        const int px = x0 + hx - kLossR, py = y0 + hy - kLossR;
        float a[3] = {0.0f, 0.0f, 0.0f}, b[3] = {0.0f, 0.0f, 0.0f};
        if (px >= 0 && py >= 0 && px < W && py < H) frame_loss_pixel<kTargetChannels>(A, (size_t)py * W + px, a, b);
#pragma unroll
        for (int c = 0; c < 3; ++c) sx[c][i] = a[c], sy[c][i] = b[c];
    }
    __syncthreads();

    float w[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) w[k] = c_loss_window[k];

    const int tx = t & (kLossTileW - 1), ty = t / kLossTileW;
    const int px = x0 + tx, py = y0 + ty;
    const bool inside = px < W && py < H;
    const size_t plane = (size_t)W * H, pix = (size_t)py * W + px;
    double sum_abs = 0.0, sum_sq = 0.0, sum_map = 0.0;

    for (int c = 0; c < 3; ++c) {
        for (int i = t; i < kLossRows; i += kLossBlock) {
            const int hy = i / kLossTileW, cx = i - hy * kLossTileW;
            const float* ax = &sx[c][hy * kLossHaloW + cx];
            const float* ay = &sy[c][hy * kLossHaloW + cx];
            float m1 = 0.0f, m2 = 0.0f, e11 = 0.0f, e22 = 0.0f, e12 = 0.0f;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const float a = ax[k], b = ay[k];
                m1 = fmaf(w[k], a, m1);
                m2 = fmaf(w[k], b, m2);
                e11 = fmaf(w[k], a * a, e11);
                e22 = fmaf(w[k], b * b, e22);
                e12 = fmaf(w[k], a * b, e12);
            }
            rows[0][i] = m1, rows[1][i] = m2, rows[2][i] = e11, rows[3][i] = e22, rows[4][i] = e12;
        }
        __syncthreads();
        float q[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 11; ++k)
#pragma unroll
            for (int j = 0; j < 5; ++j) q[j] = fmaf(w[k], rows[j][(ty + k) * kLossTileW + tx], q[j]);
        if (inside) {
            const float mu1 = q[0], mu2 = q[1];
            const float mu1mu1 = mu1 * mu1, mu2mu2 = mu2 * mu2, mu1mu2 = mu1 * mu2;
            const float s1 = q[2] - mu1mu1, s2 = q[3] - mu2mu2, s12 = q[4] - mu1mu2;
            const float A1 = 2.0f * mu1mu2 + kLossC1, A2 = 2.0f * s12 + kLossC2;
            const float B1 = (mu1mu1 + mu2mu2) + kLossC1, B2 = (s1 + s2) + kLossC2;
            const float den = B1 * B2;
            const float map = (A1 * A2) / den;
            const int centre = (ty + kLossR) * kLossHaloW + tx + kLossR;
            const float d = sx[c][centre] - sy[c][centre];
            sum_abs += (double)fabsf(d);
            sum_sq += (double)(d * d);
            sum_map += (double)map;
            if (kGrad) {
                const float d_mu = 2.0f * ((mu2 * (A2 - A1)) / den - (map * (mu1 * (B2 - B1))) / den);
                const float d_s1 = -(map / B2);
                const float d_s12 = (2.0f * A1) / den;
                maps[(size_t)(3 * c + 0) * plane + pix] = d_mu;
                maps[(size_t)(3 * c + 1) * plane + pix] = d_s1;
                maps[(size_t)(3 * c + 2) * plane + pix] = d_s12;
            }
        }
        __syncthreads();  // the row sums are overwritten by the next channel
    }

    // the lane's own pixel as a depth sample: m |D / a - t|, and 1 for the count
    double sum_depth = 0.0, sum_n = 0.0;
    if (A.depth && inside) {
        const float a = A.rgba[4 * pix + 3], td = A.target_depth[pix];
        if (frame_loss_sample(a, td, A.alpha_min)) {
            float v = fabsf(A.depth[pix] / a - td);
            if (A.mask) v = A.mask[pix] * v;
            sum_depth = (double)v;
            sum_n = 1.0;
        }
    }

    const double s_abs = loss_block_sum(sum_abs, red[0]);
    const double s_sq = loss_block_sum(sum_sq, red[1]);
    const double s_map = loss_block_sum(sum_map, red[2]);
    const double s_depth = loss_block_sum(sum_depth, red[3]);
    const double s_n = loss_block_sum(sum_n, red[4]);
    if (t == 0) {
        double* o = partial + 5 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        o[0] = s_abs, o[1] = s_sq, o[2] = s_map, o[3] = s_depth, o[4] = s_n;
    }
}

// out = {loss, l1, ssim, mse, depth_l1, depth_samples} from the tiles' five partial sums, in double, each rounded once;
// k_loss_scalars's lane assignment and tree. count = 3 H W, pixels = H W.
__global__ __launch_bounds__(256) void k_frame_scalars(uint32_t tiles, double count, double pixels, float lambda,
                                                       float depth_weight, uint32_t has_depth,
                                                       const double* __restrict__ partial, float* __restrict__ out) {
    __shared__ double part[5][256];
    const uint32_t t = threadIdx.x;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t b = t; b < tiles; b += 256)
        for (int j = 0; j < 5; ++j) s[j] += partial[5 * (size_t)b + j];
    for (int j = 0; j < 5; ++j) part[j][t] = s[j];
    __syncthreads();
    for (uint32_t off = 128; off > 0; off >>= 1) {
        if (t < off)
            for (int j = 0; j < 5; ++j) part[j][t] += part[j][t + off];
        __syncthreads();
    }
    if (t == 0) {
        const double l1 = part[0][0] / count, mse = part[1][0] / count, ssim = part[2][0] / count;
        const double depth_l1 = part[3][0] / pixels;
        const double lam = (double)lambda;
        double loss = (1.0 - lam) * l1 + lam * (1.0 - ssim);
        if (has_depth) loss += (double)depth_weight * depth_l1;
        out[0] = (float)loss;
        out[1] = (float)l1;
        out[2] = (float)ssim;
        out[3] = (float)mse;
        out[4] = (float)depth_l1;
        out[5] = (float)part[4][0];
    }
}

// k_loss_grad on x', y', then the pixel {m g_r, m g_g, m g_b, alpha slot} and the grad_depth word (gsrt.h's order)
template <int kTargetChannels>
__global__ __launch_bounds__(kLossBlock) void k_frame_grad(const FrameLossArgs A, const float* __restrict__ maps,
                                                           float scale_l1, float scale_ssim, float depth_scale,
                                                           float* __restrict__ grad, float* __restrict__ grad_depth) {
    __shared__ float sm[3][kLossHalo];
    __shared__ float rows[3][kLossRows];
    const int t = threadIdx.x;
    const int W = (int)A.W, H = (int)A.H;
    const int x0 = blockIdx.x * kLossTileW, y0 = blockIdx.y * kLossTileH;
    const int tx = t & (kLossTileW - 1), ty = t / kLossTileW;
    const int px = x0 + tx, py = y0 + ty;
    const bool inside = px < W && py < H;
    const size_t plane = (size_t)W * H, pix = (size_t)py * W + px;

    float w[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) w[k] = c_loss_window[k];

    float xv[3] = {0.0f, 0.0f, 0.0f}, yv[3] = {0.0f, 0.0f, 0.0f};
    if (inside) frame_loss_pixel<kTargetChannels>(A, pix, xv, yv);
    float g[3] = {0.0f, 0.0f, 0.0f};

    for (int c = 0; c < 3; ++c) {
        for (int i = t; i < kLossHalo; i += kLossBlock) {
            const int hy = i / kLossHaloW, hx = i - hy * kLossHaloW;
            const int qx = x0 + hx - kLossR, qy = y0 + hy - kLossR;
            const bool in = qx >= 0 && qy >= 0 && qx < W && qy < H;
            const size_t q = in ? (size_t)qy * W + qx : 0;
#pragma unroll
            for (int m = 0; m < 3; ++m) sm[m][i] = in ? maps[(size_t)(3 * c + m) * plane + q] : 0.0f;
        }
        __syncthreads();
        for (int i = t; i < kLossRows; i += kLossBlock) {
            const int hy = i / kLossTileW, cx = i - hy * kLossTileW;
            float r[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 11; ++k)
#pragma unroll
                for (int m = 0; m < 3; ++m) r[m] = fmaf(w[k], sm[m][hy * kLossHaloW + cx + k], r[m]);
#pragma unroll
            for (int m = 0; m < 3; ++m) rows[m][i] = r[m];
        }
        __syncthreads();
        float q[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 11; ++k)
#pragma unroll
            for (int m = 0; m < 3; ++m) q[m] = fmaf(w[k], rows[m][(ty + k) * kLossTileW + tx], q[m]);
        const float d = xv[c] - yv[c];
        const float sign = d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : d;  // sign(0) = 0; a NaN stays one
        const float gs = (q[0] + (2.0f * xv[c]) * q[1]) + yv[c] * q[2];
        g[c] = scale_l1 * sign - scale_ssim * gs;
        // as in k_loss_grad, the barriers above order the next channel's writes behind this channel's reads
    }
    if (!inside) return;  // no barrier follows
    const bool masked = A.mask != nullptr;
    const float m = masked ? A.mask[pix] : 1.0f;
    float ga = 0.0f, gd = 0.0f;
    if (A.has_bg) {
        const float b = (g[0] * A.bg[0] + g[1] * A.bg[1]) + g[2] * A.bg[2];
        ga = -(masked ? m * b : b);
    }
    if (A.depth) {
        const float a = A.rgba[4 * pix + 3], td = A.target_depth[pix];
        if (frame_loss_sample(a, td, A.alpha_min)) {
            const float q = A.depth[pix] / a;
            const float e = q - td;
            const float sign = e > 0.0f ? 1.0f : e < 0.0f ? -1.0f : e;
            const float s = (masked ? depth_scale * m : depth_scale) * sign;
            gd = s / a;
            ga = ga - (s * q) / a;
        }
    }
    if (masked) {
#pragma unroll
        for (int c = 0; c < 3; ++c) g[c] = m * g[c];
    }
    reinterpret_cast<float4*>(grad)[pix] = make_float4(g[0], g[1], g[2], ga);
    if (grad_depth) grad_depth[pix] = gd;
}

void launch_frame_loss(hipStream_t s, const FrameLossArgs& A, uint32_t target_channels, double* partial, float* maps,
                       float* out, float* grad, float* grad_depth) {
    const dim3 grid((A.W + kLossTileW - 1) / kLossTileW, (A.H + kLossTileH - 1) / kLossTileH);
    const bool c4 = target_channels == 4;
    if (grad) {
        if (c4) hipLaunchKernelGGL((k_frame_stats<true, 4>), grid, dim3(kLossBlock), 0, s, A, maps, partial);
        else hipLaunchKernelGGL((k_frame_stats<true, 3>), grid, dim3(kLossBlock), 0, s, A, maps, partial);
    } else {
        if (c4) hipLaunchKernelGGL((k_frame_stats<false, 4>), grid, dim3(kLossBlock), 0, s, A, maps, partial);
        else hipLaunchKernelGGL((k_frame_stats<false, 3>), grid, dim3(kLossBlock), 0, s, A, maps, partial);
    }
    const double pixels = (double)A.W * (double)A.H, count = 3.0 * pixels;
    hipLaunchKernelGGL(k_frame_scalars, dim3(1), dim3(256), 0, s, grid.x * grid.y, count, pixels, A.lambda, A.depth_weight,
                       A.depth ? 1u : 0u, partial, out);
    if (!grad) return;
    const float scale_l1 = (float)((1.0 - (double)A.lambda) / count), scale_ssim = (float)((double)A.lambda / count);
    const float depth_scale = (float)((double)A.depth_weight / pixels);
    if (c4) hipLaunchKernelGGL((k_frame_grad<4>), grid, dim3(kLossBlock), 0, s, A, maps, scale_l1, scale_ssim, depth_scale, grad, grad_depth);
    else hipLaunchKernelGGL((k_frame_grad<3>), grid, dim3(kLossBlock), 0, s, A, maps, scale_l1, scale_ssim, depth_scale, grad, grad_depth);
}

}  // namespace gsrt
