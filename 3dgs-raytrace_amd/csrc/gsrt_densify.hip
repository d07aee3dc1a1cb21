// gsrt_densify.hip -- adaptive density control on the device (gsrt_density_stats_add, gsrt_view_stats_add,
// gsrt_densify_count, gsrt_densify and their _screen forms): the densification statistic from splat rows, alone or with
// the largest screen radius beside it, the clone / split / prune / keep decision per Gaussian, and one ordered compaction
// pass that writes the new model; and gsrt_model_remap, the gather that carries the optimiser state across it.
//
// All six kernels are HBM-bound streaming kernels at ordinary priority, 256 lanes a workgroup as the scene build's
// kernels; none is a prep kernel. Per Gaussian: k_density_stats 32 B read + 8 B read-modify-write; k_view_stats the same
// and, for a seen Gaussian, its 48-B gsrt_gauss_param read + 4 B of radii read (and written when the radius grows);
// k_densify_count 24 B read (+ 4 B with radii); k_densify_write 24 B + 44 B (+ 24 B noise for a split) read, 48 B per
// output row written, plus the 192-B SH row and the feature row read once per output row and written once.
//
// The order of the output is the order of the input: Gaussian g's c_g in {0, 1, 2} rows start at o_g = sum of c_h over
// h < g. The sum has three levels: a lane's offset in its wave is two ballots and two popcounts (c >= 1 and c == 2 below
// the lane), a wave's offset in its workgroup a sum of at most three wave totals in LDS, and a workgroup's base an
// exclusive scan of the workgroup totals by one workgroup (k_densify_scan, the pattern of k_scan_digits in
// gsrt_lbvh.hip: each of 256 threads sums a run of consecutive totals, the 256 run sums are scanned in LDS). No atomics:
// the result is a pure function of the inputs.
#include <cstdint>

#include "gsrt_internal.hpp"
#include "gsrt_project.hpp"

namespace gsrt {

constexpr uint32_t kDensBlock = 256;           // lanes (Gaussians) per workgroup of the count and write kernels
constexpr uint32_t kDensWaves = kDensBlock / 64;
constexpr uint32_t kShPieces = 12;             // 16-byte pieces of a 192-byte SH row

__device__ inline uint32_t dens_popc_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// gsrt_density_stats_add: one lane per Gaussian, no atomics. The float32 operations are the header's, in its order.
__global__ __launch_bounds__(256) void k_density_stats(uint32_t n, float half_w, float half_h,
                                                       const float* __restrict__ rows, float* __restrict__ stats) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const float4* row = reinterpret_cast<const float4*>(rows) + 2 * (size_t)g;  // 32-byte rows of a 16-byte aligned table
    const float4 a = row[0], b = row[1];
    const bool seen = a.x != 0.0f || a.y != 0.0f || a.z != 0.0f || a.w != 0.0f || b.x != 0.0f || b.y != 0.0f;
    if (!seen) return;  // both words stay bit for bit as they were
    const float gx = a.x * half_w, gy = a.y * half_h;
    const float norm = sqrtf(gx * gx + gy * gy);
    float* s = stats + 2 * (size_t)g;
    s[0] = s[0] + norm;
    s[1] = s[1] + 1.0f;
}

// gsrt_view_stats_add: k_density_stats' statistic, the same operations in the same order, and beside it the largest
// screen radius (radii, nullable). One lane per Gaussian, no atomics. The loads follow what gsrt_project.hpp records for
// k_pose_partial: the row first, as two whole float4s, and the gsrt_gauss_param of a seen Gaussian only, issued with its
// radius word ahead of the statistic's read-modify-write so that the two round trips overlap. The radius
// is 3DGS's: 3 sigma of the larger eigenvalue of the chain's own V (the 0.3 low-pass included), each operation rounded on
// its own. A NaN r fails the comparison and stores nothing; an unseen, behind-camera or singular Gaussian's word is
// not touched. 25 VGPRs, no scratch: eight waves a SIMD, as k_density_stats.
__global__ __launch_bounds__(256) void k_view_stats(uint32_t n, const gsrt_ubo ubo,
                                                    const gsrt_gauss_param* __restrict__ params,
                                                    const float* __restrict__ rows, float* __restrict__ stats,
                                                    float* __restrict__ radii) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const float4* row = reinterpret_cast<const float4*>(rows) + 2 * (size_t)g;  // 32-byte rows of a 16-byte aligned table
    const float4 a = row[0], b = row[1];
    const bool seen = a.x != 0.0f || a.y != 0.0f || a.z != 0.0f || a.w != 0.0f || b.x != 0.0f || b.y != 0.0f;
    if (!seen) return;  // the statistic's words and the radius stay bit for bit as they were
    gsrt_gauss_param p;
    float have = 0.0f;
    if (radii) {
        p = params[g];  // as k_splat_grad_to_model reads it: a borrowed array need not be 16-byte aligned
        have = radii[g];
    }
    const float half_w = 0.5f * (float)ubo.width, half_h = 0.5f * (float)ubo.height;
    const float gx = a.x * half_w, gy = a.y * half_h;
    const float norm = sqrtf(gx * gx + gy * gy);
    float* s = stats + 2 * (size_t)g;
    s[0] = s[0] + norm;
    s[1] = s[1] + 1.0f;
    if (!radii) return;
    CorChain f;
    if (cor_chain(ubo, p, f) != kCorValid) return;
    const float mid = 0.5f * (f.v00 + f.v11);
    const float disc = fmaf(mid, mid, -f.det);
    const float lam = mid + sqrtf(fmaxf(0.1f, disc));
    const float r = ceilf(3.0f * sqrtf(lam));
    if (r > have) radii[g] = r;
}

// the decision of gsrt_densify for Gaussian g: its output rows (0 prune, 1 keep, 2 clone or split) and whether the two
// are split children. m is the largest scale as k_cov3d takes it. radii (nullable) with max_radius > 0: the screen-size
// prune of the _screen forms; a NaN radius fails the comparison and does not prune.
__device__ inline uint32_t densify_rows(const gsrt_densify_params& P, const float* __restrict__ scale,
                                        const float* __restrict__ opacity, const float* __restrict__ stats,
                                        const float* __restrict__ radii, float max_radius, uint32_t g, bool& split) {
    const float s0 = scale[3 * (size_t)g + 0], s1 = scale[3 * (size_t)g + 1], s2 = scale[3 * (size_t)g + 2];
    float m = s0;
    if (s1 > m) m = s1;
    if (s2 > m) m = s2;
    const float sum = stats[2 * (size_t)g + 0], cnt = stats[2 * (size_t)g + 1];
    const float mean = cnt > 0.0f ? sum / cnt : 0.0f;
    const bool prune = !(opacity[g] >= P.min_opacity) || (P.max_scale > 0.0f && m > P.max_scale) ||
                       (radii && max_radius > 0.0f && radii[g] > max_radius);
    const bool dens = !prune && mean >= P.grad_threshold;
    split = dens && m > P.split_scale;
    return prune ? 0u : dens ? 2u : 1u;
}

__global__ __launch_bounds__(kDensBlock) void k_densify_count(uint32_t n, const gsrt_densify_params P,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ opacity,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ radii, float max_radius,
                                                              uint32_t* __restrict__ block_total) {
    __shared__ uint32_t wsum[kDensWaves];
    const uint32_t t = threadIdx.x, g = blockIdx.x * kDensBlock + t;
    bool split = false;
    const uint32_t c = g < n ? densify_rows(P, scale, opacity, stats, radii, max_radius, g, split) : 0u;
    const uint64_t m1 = __ballot(c >= 1u), m2 = __ballot(c == 2u);
    if ((t & 63u) == 0) wsum[t >> 6] = (uint32_t)(__popcll(m1) + __popcll(m2));
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kDensWaves; ++w) sum += wsum[w];
        block_total[blockIdx.x] = sum;
    }
}

// One workgroup: block_total[0..nblocks) becomes its exclusive scan, *n_out the whole sum (at most 2 n < 2^32).
__global__ __launch_bounds__(256) void k_densify_scan(uint32_t nblocks, uint32_t* __restrict__ block_total,
                                                      uint32_t* __restrict__ n_out) {
    __shared__ uint32_t part[256];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nblocks + 255) / 256;
    const uint32_t b0 = min(nblocks, t * per), b1 = min(nblocks, b0 + per);
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; ++b) sum += block_total[b];
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {  // inclusive scan of the per-thread sums
        const uint32_t x = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t x = block_total[b];
        block_total[b] = run;
        run += x;
    }
    if (t == 255) *n_out = part[255];
}

// The compaction pass. Every lane recomputes its c_g, finds its first output row and writes the small fields (centre,
// rotation, scale, opacity: 11 floats) and origin of its rows itself. The SH and feature rows move workgroup-cooperatively:
// the workgroup's output rows are one contiguous run [base, base + total), each lane notes its source id for its rows in LDS
// (src[row - base]), and then consecutive lanes take consecutive 16-byte pieces of the run's SH rows (12 a row) and
// consecutive words of its feature rows: the stores are contiguous over the whole run, the loads contiguous within a
// source row, and no lane walks a 192-byte row. Indices past n * 48 are 64-bit.
// Nothing is stored when the total exceeds cap (or the largest scene): the whole grid leaves first.
__global__ __launch_bounds__(kDensBlock) void k_densify_write(uint32_t n, const gsrt_densify_params P,
                                                              const gsrt_model_arrays in, const float* __restrict__ stats,
                                                              const float* __restrict__ radii, float max_radius,
                                                              const float* __restrict__ noise, const gsrt_model_arrays out,
                                                              int32_t* __restrict__ origin, uint32_t cap,
                                                              const uint32_t* __restrict__ block_base,
                                                              const uint32_t* __restrict__ n_out) {
    __shared__ uint32_t wsum[kDensWaves];
    __shared__ uint32_t src[2 * kDensBlock];
    const uint32_t total = *n_out;
    if (total > cap || total > GSRT_MAX_GAUSSIANS) return;
    const uint32_t t = threadIdx.x, g = blockIdx.x * kDensBlock + t;
    bool split = false;
    const uint32_t c = g < n ? densify_rows(P, in.scale, in.opacity, stats, radii, max_radius, g, split) : 0u;
    const uint64_t m1 = __ballot(c >= 1u), m2 = __ballot(c == 2u);
    const uint32_t wave = t >> 6;
    if ((t & 63u) == 0) wsum[wave] = (uint32_t)(__popcll(m1) + __popcll(m2));
    __syncthreads();
    uint32_t local = dens_popc_below(m1) + dens_popc_below(m2), btotal = 0;
    for (uint32_t w = 0; w < kDensWaves; ++w) {
        if (w < wave) local += wsum[w];
        btotal += wsum[w];
    }
    const uint32_t base = block_base[blockIdx.x];
    for (uint32_t k = 0; k < c; ++k) src[local + k] = g;
    if (c) {
        // the fields as words: a copy keeps every bit, whatever the value
        const uint32_t* ic = reinterpret_cast<const uint32_t*>(in.center) + 3 * (size_t)g;
        const uint32_t* ir = reinterpret_cast<const uint32_t*>(in.rot_rxyz) + 4 * (size_t)g;
        const uint32_t* is = reinterpret_cast<const uint32_t*>(in.scale) + 3 * (size_t)g;
        const uint32_t cw[3] = {ic[0], ic[1], ic[2]}, rw[4] = {ir[0], ir[1], ir[2], ir[3]}, sw[3] = {is[0], is[1], is[2]};
        const uint32_t ow = reinterpret_cast<const uint32_t*>(in.opacity)[g];
        uint32_t ccw[2][3] = {{cw[0], cw[1], cw[2]}, {cw[0], cw[1], cw[2]}}, csw[3] = {sw[0], sw[1], sw[2]};
        if (split) {
            const float r = __uint_as_float(rw[0]), x = __uint_as_float(rw[1]), y = __uint_as_float(rw[2]),
                        z = __uint_as_float(rw[3]);
            // k_cov3d's R[c][row]: R[k][j] of gsrt.autograd.model_covariance (row k, column j) is Rc[j * 3 + k]
            const float Rc[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                                 2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                                 2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float* zn = noise + 6 * (size_t)g + 3 * k;
                const float v0 = __uint_as_float(sw[0]) * zn[0], v1 = __uint_as_float(sw[1]) * zn[1],
                            v2 = __uint_as_float(sw[2]) * zn[2];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float xj = (v0 * Rc[j * 3 + 0] + v1 * Rc[j * 3 + 1]) + v2 * Rc[j * 3 + 2];
                    ccw[k][j] = __float_as_uint(__uint_as_float(cw[j]) + xj);
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) csw[i] = __float_as_uint(__uint_as_float(sw[i]) / P.shrink);
        }
        const int32_t fresh = -1 - (int32_t)g;
        for (uint32_t k = 0; k < c; ++k) {
            const size_t o = (size_t)base + local + k;
            uint32_t* oc = reinterpret_cast<uint32_t*>(out.center) + 3 * o;
            uint32_t* orr = reinterpret_cast<uint32_t*>(out.rot_rxyz) + 4 * o;
            uint32_t* os = reinterpret_cast<uint32_t*>(out.scale) + 3 * o;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                oc[j] = ccw[k][j];
                os[j] = csw[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) orr[j] = rw[j];
            reinterpret_cast<uint32_t*>(out.opacity)[o] = ow;
            origin[o] = (split || k) ? fresh : (int32_t)g;
        }
    }
    if (!in.sh && !in.feature_channels) return;
    __syncthreads();
    if (in.sh) {
        const uint4* s = reinterpret_cast<const uint4*>(in.sh);
        uint4* d = reinterpret_cast<uint4*>(out.sh) + (size_t)base * kShPieces;
        for (uint32_t p = t; p < btotal * kShPieces; p += kDensBlock) {
            const uint32_t row = p / kShPieces, piece = p - row * kShPieces;
            d[p] = s[(size_t)src[row] * kShPieces + piece];
        }
    }
    if (const uint32_t fc = in.feature_channels) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(in.features);
        uint32_t* d = reinterpret_cast<uint32_t*>(out.features) + (size_t)base * fc;
        for (uint32_t p = t; p < btotal * fc; p += kDensBlock) {
            const uint32_t row = p / fc, word = p - row * fc;
            d[p] = s[(size_t)src[row] * fc + word];
        }
    }
}

// gsrt_model_remap: row i of every present array of `out` is row origin[i] of `in`, or +0 where origin[i] < 0: the
// optimiser state of gsrt_densify's output, all arrays in one launch. A workgroup owns 256 consecutive output rows, the
// scheme of k_densify_write's copy phase: each lane moves the small fields (11 words) of its own row, then consecutive
// lanes take consecutive pieces of the run's SH rows (WIDE: 12 uint4 pieces a row where both tables are 16-byte aligned,
// otherwise 48 words) and consecutive words of its feature rows, the source rows read from LDS. 44 B + 4 B origin read
// and 44 B written per row, plus the SH and feature rows once each way. No atomics.
template <bool WIDE>
__global__ __launch_bounds__(kDensBlock) void k_model_remap(uint32_t n_out, const int32_t* __restrict__ origin,
                                                            const gsrt_model_arrays in, const gsrt_model_arrays out) {
    __shared__ int32_t src[kDensBlock];
    const uint32_t t = threadIdx.x, base = blockIdx.x * kDensBlock, i = base + t;
    const uint32_t rows = min(kDensBlock, n_out - base);
    const int32_t g = i < n_out ? origin[i] : -1;
    src[t] = g;
    if (i < n_out) {
        const uint32_t* ic = reinterpret_cast<const uint32_t*>(in.center) + 3 * (size_t)(g < 0 ? 0 : g);
        const uint32_t* ir = reinterpret_cast<const uint32_t*>(in.rot_rxyz) + 4 * (size_t)(g < 0 ? 0 : g);
        const uint32_t* is = reinterpret_cast<const uint32_t*>(in.scale) + 3 * (size_t)(g < 0 ? 0 : g);
        uint32_t* oc = reinterpret_cast<uint32_t*>(out.center) + 3 * (size_t)i;
        uint32_t* orr = reinterpret_cast<uint32_t*>(out.rot_rxyz) + 4 * (size_t)i;
        uint32_t* os = reinterpret_cast<uint32_t*>(out.scale) + 3 * (size_t)i;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            oc[j] = g < 0 ? 0u : ic[j];
            os[j] = g < 0 ? 0u : is[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) orr[j] = g < 0 ? 0u : ir[j];
        reinterpret_cast<uint32_t*>(out.opacity)[i] = g < 0 ? 0u : reinterpret_cast<const uint32_t*>(in.opacity)[g];
    }
    if (!in.sh && !in.feature_channels) return;
    __syncthreads();
    if (in.sh) {
        if constexpr (WIDE) {
            const uint4* s = reinterpret_cast<const uint4*>(in.sh);
            uint4* d = reinterpret_cast<uint4*>(out.sh) + (size_t)base * kShPieces;
            for (uint32_t p = t; p < rows * kShPieces; p += kDensBlock) {
                const uint32_t row = p / kShPieces, piece = p - row * kShPieces;
                const int32_t h = src[row];
                d[p] = h < 0 ? make_uint4(0u, 0u, 0u, 0u) : s[(size_t)h * kShPieces + piece];
            }
        } else {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(in.sh);
            uint32_t* d = reinterpret_cast<uint32_t*>(out.sh) + (size_t)base * 48;
            for (uint32_t p = t; p < rows * 48u; p += kDensBlock) {
                const uint32_t row = p / 48u, word = p - row * 48u;
                const int32_t h = src[row];
                d[p] = h < 0 ? 0u : s[(size_t)h * 48 + word];
            }
        }
    }
    if (const uint32_t fc = in.feature_channels) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(in.features);
        uint32_t* d = reinterpret_cast<uint32_t*>(out.features) + (size_t)base * fc;
        for (uint32_t p = t; p < rows * fc; p += kDensBlock) {
            const uint32_t row = p / fc, word = p - row * fc;
            const int32_t h = src[row];
            d[p] = h < 0 ? 0u : s[(size_t)h * fc + word];
        }
    }
}

void launch_model_remap(hipStream_t s, uint32_t n_out, const int32_t* origin, const gsrt_model_arrays& in,
                        const gsrt_model_arrays& out) {
    const uint32_t nblocks = densify_blocks(n_out);
    if (!nblocks) return;
    const bool wide = (reinterpret_cast<uintptr_t>(in.sh) | reinterpret_cast<uintptr_t>(out.sh)) % 16u == 0;
    if (wide)
        hipLaunchKernelGGL(k_model_remap<true>, dim3(nblocks), dim3(kDensBlock), 0, s, n_out, origin, in, out);
    else
        hipLaunchKernelGGL(k_model_remap<false>, dim3(nblocks), dim3(kDensBlock), 0, s, n_out, origin, in, out);
}

uint32_t densify_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + kDensBlock - 1) / kDensBlock); }

void launch_density_stats(hipStream_t s, uint32_t n, uint32_t width, uint32_t height, const float* rows, float* stats) {
    if (!n) return;
    hipLaunchKernelGGL(k_density_stats, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, s, n,
                       0.5f * (float)width, 0.5f * (float)height, rows, stats);
}

void launch_view_stats(hipStream_t s, uint32_t n, const gsrt_ubo& ubo, const gsrt_gauss_param* params, const float* rows,
                       float* stats, float* radii) {
    if (!n) return;
    hipLaunchKernelGGL(k_view_stats, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, s, n, ubo, params, rows,
                       stats, radii);
}

void launch_densify_count(hipStream_t s, uint32_t n, const gsrt_densify_params& P, const float* scale, const float* opacity,
                          const float* stats, const float* radii, float max_radius, uint32_t* block_total,
                          uint32_t* d_n_out) {
    const uint32_t nblocks = densify_blocks(n);
    if (nblocks)
        hipLaunchKernelGGL(k_densify_count, dim3(nblocks), dim3(kDensBlock), 0, s, n, P, scale, opacity, stats, radii,
                           max_radius, block_total);
    hipLaunchKernelGGL(k_densify_scan, dim3(1), dim3(256), 0, s, nblocks, block_total, d_n_out);
}

void launch_densify_write(hipStream_t s, uint32_t n, const gsrt_densify_params& P, const gsrt_model_arrays& in,
                          const float* stats, const float* radii, float max_radius, const float* noise,
                          const gsrt_model_arrays& out, int32_t* origin, uint32_t cap, const uint32_t* block_base,
                          const uint32_t* d_n_out) {
    const uint32_t nblocks = densify_blocks(n);
    if (!nblocks) return;
    hipLaunchKernelGGL(k_densify_write, dim3(nblocks), dim3(kDensBlock), 0, s, n, P, in, stats, radii, max_radius, noise,
                       out, origin, cap, block_base, d_n_out);
}

}  // namespace gsrt
