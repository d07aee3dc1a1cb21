// gsrt_cov3d.hpp -- one Gaussian of the scene build: Gauss::init_cov3d / init_radius / BoundingBox
// (RayTracingInVulkan/src/Assets/Sphere.hpp:108-165), packed as Scene.cpp:125-136 does. The body of k_cov3d
// (gsrt_scene.hip), shared with the model step (gsrt_model_step.hip), whose scene arrays are the scene build's bit for bit.
#pragma once
#include "gsrt_internal.hpp"

namespace gsrt {

// centre c, rotation (r, x, y, z) used as given, scales s, opacity o. glm mat3 products are summed left to right.
__device__ GSRT_INLINE void cov3d_pack(const float c[3], float r, float x, float y, float z, float s0, float s1, float s2,
                                       float o, gsrt_gauss_param& g, gsrt_aabb& a) {
    // R[c][row], glm::mat3 column-major constructor (Sphere.hpp:143-147)
    float R[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                  2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                  2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)};
    const float S[9] = {s0, 0.f, 0.f, 0.f, s1, 0.f, 0.f, 0.f, s2};
    float M[9];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            M[c * 3 + k] = (S[0 * 3 + k] * R[c * 3 + 0] + S[1 * 3 + k] * R[c * 3 + 1]) + S[2 * 3 + k] * R[c * 3 + 2];
    // Sigma = transpose(M) * M: Sigma[c][k] = (Mt[0][k]*M[c][0] + Mt[1][k]*M[c][1]) + Mt[2][k]*M[c][2], Mt[a][k] = M[k][a]
    float Sig[9];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            Sig[c * 3 + k] = (M[k * 3 + 0] * M[c * 3 + 0] + M[k * 3 + 1] * M[c * 3 + 1]) + M[k * 3 + 2] * M[c * 3 + 2];
    g.center_opacity[0] = c[0];
    g.center_opacity[1] = c[1];
    g.center_opacity[2] = c[2];
    g.center_opacity[3] = o;
    g.cov3d[0] = Sig[0]; g.cov3d[1] = Sig[1]; g.cov3d[2] = Sig[2];
    g.cov3d[3] = Sig[4]; g.cov3d[4] = Sig[5]; g.cov3d[5] = Sig[8];
    g.pad[0] = 0.f; g.pad[1] = 0.f;
    float mx = s0;
    if (s1 > mx) mx = s1;
    if (s2 > mx) mx = s2;
    const float rad = (float)(3.0 * (double)mx);  // Sphere.hpp:164, double product stored as float
    a.min_x = g.center_opacity[0] - rad; a.min_y = g.center_opacity[1] - rad; a.min_z = g.center_opacity[2] - rad;
    a.max_x = g.center_opacity[0] + rad; a.max_y = g.center_opacity[1] + rad; a.max_z = g.center_opacity[2] + rad;
}

}  // namespace gsrt
