// gsrt_model_step.hip -- the optimiser step on the device (gsrt_model_step, gsrt_model_activate, gsrt_model_deactivate,
// gsrt_model_opacity_reset): the chain from the library's gradient tables to the raw parameters (unnormalised quaternion,
// log scale, logit opacity), Adam, and the next frame's arrays (the activated model, gsrt_gauss_param rows, gsrt_aabb boxes).
//
// Two HBM-bound streaming kernels, 256 lanes a workgroup at ordinary priority as the scene build's and densify's; no LDS,
// no atomics: the result is a pure function of the inputs.
//
// k_model_geom: one lane per Gaussian. A stepped Gaussian moves 11 words of raw, m and v in and out (132 B + 132 B), 68 B
// of gradients in (centre 12, cov 24, splat row 32), and 72 B of scene arrays out, + 44 B for act and 44 B for grad_raw when
// asked for. The 16-, 32- and 48-byte rows (rot and its moments, the splat row, gsrt_gauss_param) move as whole float4s
// and the 24-byte rows (cov, gsrt_aabb) as float2s when every such base is aligned for it (VEC); the 12-byte rows (centre,
// scale) and the 44-byte grad_raw rows are three and eleven dword accesses a lane: a wave's three loads together still
// cover one contiguous 768-byte run. 73 VGPRs, no scratch: six waves a SIMD under __launch_bounds__(256), enough to hide
// HBM latency for a lane that issues its ~20 loads in three dependent groups (raw and the splat row; gradients; moments).
// k_model_rows takes 32 VGPRs: eight waves a SIMD.
//
// k_model_rows: the SH and feature rows, flat over the table's words, one float4 a lane (W = 4), so that a wave's access is
// one contiguous KiB whatever the row length; the Gaussian and the word in its row come from the flat index (a float4 never
// straddles two rows: 48 and C are multiples of 4 on this path). One word a lane (the scalar path) for C not a multiple
// of 4 or a base that is not 16-byte aligned. Sparse: a lane reads its Gaussian's splat row (the 12 lanes of an SH row
// read the same 32 bytes: one line from L1) and leaves without touching raw, m, v when it was not seen. Per stepped
// word: raw, m, v and the gradient in, raw, m, v out (16 B + 12 B), + 4 B out for act rows.
//
// The float32 operations are the ones written here, each rounded on its own (the library is built with
// -ffp-contract=off and correctly rounded division and square root); include/gsrt.h states them.
#include <cstdint>

#include "gsrt_cov3d.hpp"
#include "gsrt_internal.hpp"

namespace gsrt {

__device__ GSRT_INLINE void adam_word(const AdamScalars& K, float ss, float g, float& p, float& m, float& v) {
    m = K.beta1 * m + K.a1 * g;
    v = K.beta2 * v + (K.a2 * g) * g;
    p = p - (ss * m) / (sqrtf(v) / K.c2 + K.eps);
}

// "seen" as gsrt_density_stats_add defines it: any of row[0..5] != 0.0f (a -0 is not seen, a NaN is)
__device__ GSRT_INLINE bool row_seen(const float r[6]) {
    return r[0] != 0.0f || r[1] != 0.0f || r[2] != 0.0f || r[3] != 0.0f || r[4] != 0.0f || r[5] != 0.0f;
}

template <bool VEC>
__device__ GSRT_INLINE void load_splat6(const float* __restrict__ splat, size_t g, float r[6]) {
    if constexpr (VEC) {
        const float4 a = reinterpret_cast<const float4*>(splat)[2 * g];
        const float2 b = reinterpret_cast<const float2*>(splat)[4 * g + 2];
        r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w; r[4] = b.x; r[5] = b.y;
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) r[k] = splat[8 * g + k];
    }
}

template <bool VEC>
__device__ GSRT_INLINE void load4(const float* p, size_t g, float o[4]) {
    if constexpr (VEC) {
        const float4 a = reinterpret_cast<const float4*>(p)[g];
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = p[4 * g + k];
    }
}

template <bool VEC>
__device__ GSRT_INLINE void store4(float* p, size_t g, const float o[4]) {
    if constexpr (VEC) reinterpret_cast<float4*>(p)[g] = make_float4(o[0], o[1], o[2], o[3]);
    else {
#pragma unroll
        for (int k = 0; k < 4; ++k) p[4 * g + k] = o[k];
    }
}

template <bool VEC>
__device__ GSRT_INLINE void load6(const float* p, size_t g, float o[6]) {
    if constexpr (VEC) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float2 a = reinterpret_cast<const float2*>(p)[3 * g + k];
            o[2 * k] = a.x; o[2 * k + 1] = a.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = p[6 * g + k];
    }
}

__device__ GSRT_INLINE void load3(const float* p, size_t g, float o[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = p[3 * g + k];
}

__device__ GSRT_INLINE void store3(float* p, size_t g, const float o[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[3 * g + k] = o[k];
}

// The activation of gsrt.h: nq (1 + 3 + 1 rounded operations), q = raw / nq (nq == 0 leaves raw), s = expf(log scale),
// o = 1 / (1 + expf(-logit))
__device__ GSRT_INLINE void activate(const float raw_q[4], const float ls[3], float lo, float& nq, float q[4], float s[3],
                                     float& o) {
    nq = sqrtf(((raw_q[0] * raw_q[0] + raw_q[1] * raw_q[1]) + raw_q[2] * raw_q[2]) + raw_q[3] * raw_q[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = nq == 0.0f ? raw_q[k] : raw_q[k] / nq;
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = expf(ls[k]);
    o = 1.0f / (1.0f + expf(-lo));
}

// The chain of gsrt.h from dL/d(cov3d) (dcov, cov3d's order: an off-diagonal slot is one variable) and the splat row's
// slot 5 to the raw parameters. R[k][i] (row k, column i) is the matrix of Sigma_ij = sum_k s_k^2 R_ki R_kj, the scene
// build's polynomial in q. With D the symmetric dL/dSigma (an off-diagonal entry half its slot: exact), w_k = D R_k:
//   dL/ds_k = 2 s_k (R_k . w_k),  dL/dR_ka = 2 s_k^2 w_ka,  dL/dq_c = sum_ka dL/dR_ka dR_ka/dq_c,
// the sums tests/cor_f64_geom.py's param_chain forms. Rounded operations on the longest path from the raw inputs, a
// product counting one more than its factors together, E the error of expf in units of 2^-24 (tests/model_step_ref.py):
//   q 6 (nq 5, the division 1); R 15 (a product of two q 13, the sum 14, 1 - 2 (.) 15); w 18 (D R 16, three terms);
//   R_k . w_k 36; dL/ds_k = (2 s_k) (.) E + 37; d log scale = dL/ds_k s_k: 2 E + 38.
//   2 s_k^2: 2 E + 1; dL/dR: 2 E + 20; a sum or difference of two: 2 E + 21; times a q: 2 E + 28; four terms: dL/dq 2 E + 31;
//   q . dq: 2 E + 41; q (q . dq): 2 E + 48; dq - (.): 2 E + 49; / nq: 2 E + 55.
//   o: E + 2; 1 - o: E + 3 of (1 + o); (d o) (1 - o): 2 E + 7.
__device__ GSRT_INLINE void chain_raw(const float dcov[6], float dop, float nq, const float q[4], const float s[3], float o,
                                      float d_rot[4], float d_ls[3], float& d_logit) {
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    const float R[3][3] = {{1.f - 2.f * (y * y + z * z), 2.f * (x * y + r * z), 2.f * (x * z - r * y)},
                           {2.f * (x * y - r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z + r * x)},
                           {2.f * (x * z + r * y), 2.f * (y * z - r * x), 1.f - 2.f * (x * x + y * y)}};
    const float h01 = 0.5f * dcov[1], h02 = 0.5f * dcov[2], h12 = 0.5f * dcov[4];
    const float D[3][3] = {{dcov[0], h01, h02}, {h01, dcov[3], h12}, {h02, h12, dcov[5]}};
    float gR[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float w[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) w[a] = (D[a][0] * R[k][0] + D[a][1] * R[k][1]) + D[a][2] * R[k][2];
        const float t = (R[k][0] * w[0] + R[k][1] * w[1]) + R[k][2] * w[2];
        const float s2 = 2.f * s[k];
        d_ls[k] = (s2 * t) * s[k];
        const float h = s2 * s[k];
#pragma unroll
        for (int a = 0; a < 3; ++a) gR[k][a] = h * w[a];
    }
    // dR/dq_c entry by entry (tests/cor_f64_geom.py _rotation): every entry is +-2 or +-4 times one component of q
    const float a01 = gR[0][1] + gR[1][0], a02 = gR[0][2] + gR[2][0], a12 = gR[1][2] + gR[2][1];
    const float b01 = gR[0][1] - gR[1][0], b20 = gR[2][0] - gR[0][2], b12 = gR[1][2] - gR[2][1];
    float dq[4];
    dq[0] = 2.f * ((z * b01 + y * b20) + x * b12);
    dq[1] = 2.f * (((y * a01 + z * a02) + r * b12) - (2.f * x) * (gR[1][1] + gR[2][2]));
    dq[2] = 2.f * (((x * a01 + r * b20) + z * a12) - (2.f * y) * (gR[0][0] + gR[2][2]));
    dq[3] = 2.f * (((r * b01 + x * a02) + y * a12) - (2.f * z) * (gR[0][0] + gR[1][1]));
    const float qd = ((q[0] * dq[0] + q[1] * dq[1]) + q[2] * dq[2]) + q[3] * dq[3];
#pragma unroll
    for (int c = 0; c < 4; ++c) d_rot[c] = nq == 0.0f ? 0.0f : (dq[c] - q[c] * qd) / nq;
    d_logit = (dop * o) * (1.0f - o);
}

// STEP: the chain and Adam before the activation; without it the activation and packing alone (gsrt_model_activate), the
// same code. act members, params, aabbs and grad_raw are each nullable.
template <bool STEP, bool VEC>
__global__ __launch_bounds__(256) void k_model_geom(uint32_t n, const AdamScalars K, const gsrt_model_arrays raw,
                                                    const gsrt_model_arrays mom1, const gsrt_model_arrays mom2,
                                                    const gsrt_model_grads G, const gsrt_model_arrays act,
                                                    gsrt_gauss_param* params, gsrt_aabb* aabbs, float* grad_raw) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    float c[3], rq[4], ls[3], lo;
    load3(raw.center, g, c);
    load4<VEC>(raw.rot_rxyz, g, rq);
    load3(raw.scale, g, ls);
    lo = raw.opacity[g];
    float nq, q[4], s[3], o;
    if constexpr (STEP) {
        float row[6];
        load_splat6<VEC>(G.splat, g, row);
        const bool stepped = !(K.flags & GSRT_ADAM_SPARSE) || row_seen(row);
        if (stepped || grad_raw) {
            activate(rq, ls, lo, nq, q, s, o);
            float dc[3], dcov[6], d_rot[4], d_ls[3], d_logit;
            load3(G.center, g, dc);
            load6<VEC>(G.cov, g, dcov);
            chain_raw(dcov, row[5], nq, q, s, o, d_rot, d_ls, d_logit);
            if (grad_raw) {
                float* o11 = grad_raw + 11 * g;
#pragma unroll
                for (int k = 0; k < 3; ++k) o11[k] = dc[k];
#pragma unroll
                for (int k = 0; k < 4; ++k) o11[3 + k] = d_rot[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) o11[7 + k] = d_ls[k];
                o11[10] = d_logit;
            }
            if (stepped) {
                if (!(K.frozen & 1u)) {
                    float m[3], v[3];
                    load3(mom1.center, g, m);
                    load3(mom2.center, g, v);
#pragma unroll
                    for (int k = 0; k < 3; ++k) adam_word(K, K.ss[0], dc[k], c[k], m[k], v[k]);
                    store3(raw.center, g, c);
                    store3(mom1.center, g, m);
                    store3(mom2.center, g, v);
                }
                if (!(K.frozen & 2u)) {
                    float m[4], v[4];
                    load4<VEC>(mom1.rot_rxyz, g, m);
                    load4<VEC>(mom2.rot_rxyz, g, v);
#pragma unroll
                    for (int k = 0; k < 4; ++k) adam_word(K, K.ss[1], d_rot[k], rq[k], m[k], v[k]);
                    store4<VEC>(raw.rot_rxyz, g, rq);
                    store4<VEC>(mom1.rot_rxyz, g, m);
                    store4<VEC>(mom2.rot_rxyz, g, v);
                }
                if (!(K.frozen & 4u)) {
                    float m[3], v[3];
                    load3(mom1.scale, g, m);
                    load3(mom2.scale, g, v);
#pragma unroll
                    for (int k = 0; k < 3; ++k) adam_word(K, K.ss[2], d_ls[k], ls[k], m[k], v[k]);
                    store3(raw.scale, g, ls);
                    store3(mom1.scale, g, m);
                    store3(mom2.scale, g, v);
                }
                if (!(K.frozen & 8u)) {
                    float m = mom1.opacity[g], v = mom2.opacity[g];
                    adam_word(K, K.ss[3], d_logit, lo, m, v);
                    raw.opacity[g] = lo;
                    mom1.opacity[g] = m;
                    mom2.opacity[g] = v;
                }
            }
        }
    }
    activate(rq, ls, lo, nq, q, s, o);  // from the updated raw values
    if (act.center) store3(act.center, g, c);
    if (act.rot_rxyz) store4<VEC>(act.rot_rxyz, g, q);
    if (act.scale) store3(act.scale, g, s);
    if (act.opacity) act.opacity[g] = o;
    if (params || aabbs) {
        gsrt_gauss_param gp;
        gsrt_aabb box;
        cov3d_pack(c, q[0], q[1], q[2], q[3], s[0], s[1], s[2], o, gp, box);
        if (params) {
            if constexpr (VEC) {
                float4* d = reinterpret_cast<float4*>(params) + 3 * g;
                d[0] = make_float4(gp.center_opacity[0], gp.center_opacity[1], gp.center_opacity[2], gp.center_opacity[3]);
                d[1] = make_float4(gp.cov3d[0], gp.cov3d[1], gp.cov3d[2], gp.cov3d[3]);
                d[2] = make_float4(gp.cov3d[4], gp.cov3d[5], gp.pad[0], gp.pad[1]);
            } else params[g] = gp;
        }
        if (aabbs) {
            if constexpr (VEC) {
                float2* d = reinterpret_cast<float2*>(aabbs) + 3 * g;
                d[0] = make_float2(box.min_x, box.min_y);
                d[1] = make_float2(box.min_z, box.max_x);
                d[2] = make_float2(box.max_y, box.max_z);
            } else aabbs[g] = box;
        }
    }
}

// The SH (len 48: words 0..2 of a row are coefficient 0, group ss_head) or feature rows (len C, one group), flat over
// the table. W = 4: one float4 a lane (len a multiple of 4, 16-byte aligned bases); W = 1: one word a lane.
// frozen_head / frozen_rest: that group's words keep their bits. limit: so do the words from `limit` on of a row (the SH
// words above the active degree, 3 (d + 1)^2 of 48; len: none). The test is per word: 3, 12 and 27 are no multiples
// of 4, so a W == 4 lane can straddle the limit; a lane wholly past it touches m, v and the gradient no more than an
// unseen Gaussian's does. act_rows (nullable): the updated words are stored there too, for every Gaussian.
template <int W>
__global__ __launch_bounds__(256) void k_model_rows(size_t count, uint32_t len, uint32_t head, uint32_t limit,
                                                    const AdamScalars K, float ss_head, float ss_rest,
                                                    uint32_t frozen_head, uint32_t frozen_rest, float* raw, float* mom1,
                                                    float* mom2,
                                                    const float* __restrict__ grad, const float* __restrict__ splat,
                                                    uint32_t splat_vec, float* act_rows) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const size_t w0 = i * W, g = w0 / len;
    const uint32_t wi = (uint32_t)(w0 - g * len);
    bool stepped = wi < limit;
    if (stepped && (K.flags & GSRT_ADAM_SPARSE)) {
        float row[6];
        if (splat_vec) load_splat6<true>(splat, g, row);
        else load_splat6<false>(splat, g, row);
        stepped = row_seen(row);
    }
    if (!stepped && !act_rows) return;
    float p[W], m[W], v[W], gr[W];
    if constexpr (W == 4) {
        const float4 a = reinterpret_cast<const float4*>(raw)[i];
        p[0] = a.x; p[1] = a.y; p[2] = a.z; p[3] = a.w;
    } else p[0] = raw[i];
    if (stepped) {
        if constexpr (W == 4) {
            const float4 a = reinterpret_cast<const float4*>(mom1)[i], b = reinterpret_cast<const float4*>(mom2)[i],
                         d = reinterpret_cast<const float4*>(grad)[i];
            m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w;
            v[0] = b.x; v[1] = b.y; v[2] = b.z; v[3] = b.w;
            gr[0] = d.x; gr[1] = d.y; gr[2] = d.z; gr[3] = d.w;
        } else {
            m[0] = mom1[i]; v[0] = mom2[i]; gr[0] = grad[i];
        }
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const bool is_head = wi + j < head;
            if ((is_head ? frozen_head : frozen_rest) || wi + j >= limit) continue;  // the words keep their bits
            adam_word(K, is_head ? ss_head : ss_rest, gr[j], p[j], m[j], v[j]);
        }
        if constexpr (W == 4) {
            reinterpret_cast<float4*>(raw)[i] = make_float4(p[0], p[1], p[2], p[3]);
            reinterpret_cast<float4*>(mom1)[i] = make_float4(m[0], m[1], m[2], m[3]);
            reinterpret_cast<float4*>(mom2)[i] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            raw[i] = p[0]; mom1[i] = m[0]; mom2[i] = v[0];
        }
    }
    if (act_rows) {
        if constexpr (W == 4) reinterpret_cast<float4*>(act_rows)[i] = make_float4(p[0], p[1], p[2], p[3]);
        else act_rows[i] = p[0];
    }
}

// gsrt_model_deactivate: one lane per Gaussian; centre and rotation copied as words
__global__ __launch_bounds__(256) void k_model_deactivate(uint32_t n, const gsrt_model_arrays act, const gsrt_model_arrays raw) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const uint32_t* ic = reinterpret_cast<const uint32_t*>(act.center) + 3 * g;
    const uint32_t* ir = reinterpret_cast<const uint32_t*>(act.rot_rxyz) + 4 * g;
    uint32_t* oc = reinterpret_cast<uint32_t*>(raw.center) + 3 * g;
    uint32_t* orr = reinterpret_cast<uint32_t*>(raw.rot_rxyz) + 4 * g;
#pragma unroll
    for (int k = 0; k < 3; ++k) oc[k] = ic[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) orr[k] = ir[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) raw.scale[3 * g + k] = logf(act.scale[3 * g + k]);
    const float o = act.opacity[g];
    raw.opacity[g] = logf(o / (1.0f - o));
}

// gsrt_model_opacity_reset: one lane per Gaussian; a NaN logit fails the comparison and stays
__global__ __launch_bounds__(256) void k_opacity_reset(uint32_t n, float limit, float* logit, float* m, float* v) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const float l = logit[g];
    if (l > limit) logit[g] = limit;
    m[g] = 0.0f;
    v[g] = 0.0f;
}

static uint32_t blocks256(size_t count) { return (uint32_t)((count + 255) / 256); }

static bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// one table of rows: the float4 path when the row length and every base allow it
static void launch_rows(hipStream_t s, uint32_t n, uint32_t len, uint32_t head, uint32_t limit, const AdamScalars& K,
                        float ss_head, float ss_rest, bool frozen_head, bool frozen_rest, float* raw, float* m, float* v,
                        const float* grad, const float* splat, float* act_rows) {
    const size_t words = (size_t)n * len;
    const bool vec = len % 4 == 0 && aligned(raw, 16) && aligned(m, 16) && aligned(v, 16) && aligned(grad, 16) &&
                     aligned(act_rows, 16);
    const uint32_t splat_vec = aligned(splat, 16) ? 1u : 0u;
    if (vec)
        hipLaunchKernelGGL(k_model_rows<4>, dim3(blocks256(words / 4)), dim3(256), 0, s, words / 4, len, head, limit, K,
                           ss_head, ss_rest, frozen_head ? 1u : 0u, frozen_rest ? 1u : 0u, raw, m, v, grad, splat, splat_vec,
                           act_rows);
    else
        hipLaunchKernelGGL(k_model_rows<1>, dim3(blocks256(words)), dim3(256), 0, s, words, len, head, limit, K, ss_head,
                           ss_rest, frozen_head ? 1u : 0u, frozen_rest ? 1u : 0u, raw, m, v, grad, splat, splat_vec, act_rows);
}

void launch_model_step(hipStream_t s, uint32_t n, const AdamScalars* K, const gsrt_model_arrays& raw,
                       const gsrt_model_arrays* m, const gsrt_model_arrays* v, const gsrt_model_grads* G,
                       const gsrt_model_arrays& act, gsrt_gauss_param* params, gsrt_aabb* aabbs, float* grad_raw,
                       uint32_t sh_degree) {
    if (!n) return;
    bool vec = aligned(raw.rot_rxyz, 16) && aligned(act.rot_rxyz, 16) && aligned(params, 16) && aligned(aabbs, 8);
    if (K)
        vec = vec && aligned(m->rot_rxyz, 16) && aligned(v->rot_rxyz, 16) && aligned(G->splat, 16) && aligned(G->cov, 8);
    const dim3 grid(blocks256(n)), block(256);
    const gsrt_model_arrays none{};
    const gsrt_model_grads no_grads{};
    if (K) {
        if (vec) hipLaunchKernelGGL((k_model_geom<true, true>), grid, block, 0, s, n, *K, raw, *m, *v, *G, act, params, aabbs, grad_raw);
        else hipLaunchKernelGGL((k_model_geom<true, false>), grid, block, 0, s, n, *K, raw, *m, *v, *G, act, params, aabbs, grad_raw);
    } else {
        const AdamScalars zero{};
        if (vec) hipLaunchKernelGGL((k_model_geom<false, true>), grid, block, 0, s, n, zero, raw, none, none, no_grads, act, params, aabbs, nullptr);
        else hipLaunchKernelGGL((k_model_geom<false, false>), grid, block, 0, s, n, zero, raw, none, none, no_grads, act, params, aabbs, nullptr);
    }
    // the rows: stepped where a group moves, copied to act where it is another array
    struct Table { float* raw; float* m; float* v; const float* grad; float* act; uint32_t len, head, limit; int g_head, g_rest; };
    const uint32_t sh_words = 3u * (sh_degree + 1u) * (sh_degree + 1u);  // the active words of an SH row
    const Table tables[2] = {
        {raw.sh, K ? m->sh : nullptr, K ? v->sh : nullptr, K ? G->sh : nullptr, act.sh, 48u, 3u, sh_words, 4, 5},
        {raw.features, K ? m->features : nullptr, K ? v->features : nullptr, K ? G->features : nullptr, act.features,
         raw.feature_channels, 0u, raw.feature_channels, 6, 6}};
    for (const Table& t : tables) {
        if (!t.raw) continue;
        float* const act_rows = t.act && t.act != t.raw ? t.act : nullptr;
        const bool fh = !K || ((K->frozen >> t.g_head) & 1u);
        const bool fr = !K || ((K->frozen >> t.g_rest) & 1u) || t.limit <= t.head;  // degree 0: no word of the rest moves
        if (K && !(fh && fr))
            launch_rows(s, n, t.len, t.head, t.limit, *K, K->ss[t.g_head], K->ss[t.g_rest], fh, fr, t.raw, t.m, t.v, t.grad,
                        G->splat, act_rows);
        else if (act_rows)
            (void)hipMemcpyAsync(act_rows, t.raw, sizeof(float) * (size_t)n * t.len, hipMemcpyDeviceToDevice, s);
    }
}

void launch_model_deactivate(hipStream_t s, uint32_t n, const gsrt_model_arrays& act, const gsrt_model_arrays& raw) {
    if (!n) return;
    hipLaunchKernelGGL(k_model_deactivate, dim3(blocks256(n)), dim3(256), 0, s, n, act, raw);
    if (act.sh && act.sh != raw.sh)
        (void)hipMemcpyAsync(raw.sh, act.sh, sizeof(float) * 48 * (size_t)n, hipMemcpyDeviceToDevice, s);
    if (act.features && act.features != raw.features)
        (void)hipMemcpyAsync(raw.features, act.features, sizeof(float) * (size_t)n * act.feature_channels,
                             hipMemcpyDeviceToDevice, s);
}

void launch_opacity_reset(hipStream_t s, uint32_t n, float limit, float* logit, float* m, float* v) {
    if (!n) return;
    hipLaunchKernelGGL(k_opacity_reset, dim3(blocks256(n)), dim3(256), 0, s, n, limit, logit, m, v);
}

}  // namespace gsrt
