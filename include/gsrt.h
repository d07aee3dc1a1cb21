/*
 * gsrt.h -- C ABI of the MI355X-native ray-traced 3D Gaussian Splatting renderer.
 *
 * This header is the drop-in surface a reference-side caller links against. The library's test and measurement hooks
 * (host mirrors of the sharded layout, emulated gathers, diagnostic counters, synthetic clouds, the test switches)
 * are declared separately in gsrt_test.h.
 *
 * Drop-in boundary for the reference's Gaussian render path. The
 * reference path is reached through three nested boundaries; each entry point below
 * names the reference interface it replaces (paths relative to the reference root):
 *
 *   scene upload   Assets::Scene ctor packing GaussParam/AABB/NextK/RayInfo/ExpLUT
 *                  (RayTracingInVulkan/src/Assets/Scene.cpp:16-182)
 *   AS build       vkCmdBuildAccelerationStructuresKHR -> lvp_cpu_build_acceleration_structures
 *                  (mesa-vulkan-sim/src/gallium/frontends/lavapipe/lvp_acceleration_structure.c:1182-1400)
 *   dispatch       vkCmdTraceRaysKHR(W,H,1) -> gpgpusim_vkCmdTraceRaysKHR
 *                  (vulkan-sim/src/cuda-sim/gpgpusim_calls_from_mesa.cc:60-74)
 *   frame dump     VulkanRayTracing::image_store P3 PPM (vulkan-sim/src/cuda-sim/vulkan_ray_tracing.cc:2203-2247)
 *
 * Conventions: every call returns a gsrt_status (no exceptions cross the ABI); input
 * arrays are copied (the caller keeps ownership); scene objects are owned by the library;
 * one gsrt_ctx per device; calls on one ctx are serialised by the caller.
 */
#ifndef GSRT_H
#define GSRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSRT_ABI_VERSION 2
/* largest scene: Gaussian ids are 31-bit (BVH child refs use bit 31 as the leaf flag) */
#define GSRT_MAX_GAUSSIANS 0x7fffffffu

typedef struct gsrt_ctx gsrt_ctx;
typedef struct gsrt_scene gsrt_scene;

typedef enum {
    GSRT_OK = 0,
    GSRT_E_ARG = -1,     /* bad argument (null pointer, size mismatch, unsupported mode) */
    GSRT_E_OOM = -2,     /* device or host allocation failed */
    GSRT_E_DEVICE = -3,  /* HIP runtime / kernel failure, or no device */
    GSRT_E_IO = -4,      /* file open/read/write failed */
    GSRT_E_STATE = -5,   /* call out of order (e.g. render before gsrt_build_bvh) */
    GSRT_E_COMM = -6     /* RCCL failure */
} gsrt_status;

/* == GaussParam (RayTracingInVulkan/assets/shaders/Gauss.glsl:1-6; Assets/Sphere.hpp:10-19), 48 B */
typedef struct { float center_opacity[4]; float cov3d[6]; float pad[2]; } gsrt_gauss_param;
/* == VkAabbPositionsKHR as packed by Scene.cpp:129-130, 24 B */
typedef struct { float min_x, min_y, min_z, max_x, max_y, max_z; } gsrt_aabb;
/* == UniformBufferObject (Assets/UniformBuffer.hpp:15-36; shaders/UniformBufferObject.glsl), 320 B,
 *    matrices column-major (glm layout) */
typedef struct {
    float model_view[16], projection[16], model_view_inverse[16], projection_inverse[16];
    float light_position[3], light_radius, aperture, focus_distance, heatmap_scale;
    uint32_t total_samples, samples, bounces, shadows, random_seed, width, height, has_sky, show_heatmap;
} gsrt_ubo;
/* Per-ray state after the frame: RayInfo {Depth, GaussNum} (RayPayload.glsl:11-16), Ray.Trans,
 * NextK[ray][8] {depth, alpha} (Gauss.glsl:8-12). gauss_num is clamped to 8; gauss_num_raw is the
 * unclamped insert count of the last round (the reference indexes NextK with it, rchit:23-31). 80 B */
typedef struct { float trans; float depth; int32_t gauss_num; int32_t gauss_num_raw; float k[8][2]; } gsrt_raystate;

/* render modes */
enum {
    GSRT_MODE_REF = 0,      /* bit-faithful restatement of GaussTracing.rgen/.rint/.rchit (K=8 rounds) */
    GSRT_MODE_COR = 1,      /* front-facing depth, conic = (V+0.3I)^-1, exp, alpha<=0.99, SH-3 colour,
                               depth-ordered blend, early stop at T<1e-4, jittered spp */
    GSRT_FLAG_LUT = 0x100,  /* COR: use the reference LinearExp LUT (ExpLUT.hpp) instead of exp */
    GSRT_FLAG_STATS = 0x200, /* also count candidates / blended hits (gsrt_last_stats) */
    GSRT_FLAG_OUT_DUMP8 = 0x400, /* sharded COR frames: exchange and keep the frame as the integers its PPM dump prints
                                   (gsrt_dump8_*), 4 bytes per pixel instead of RGBA32F's 16 */
    GSRT_FLAG_DEPTH = 0x800, /* whole COR frames: also write the expected view depth per pixel (gsrt_render_depth below);
                               GSRT_E_ARG with REF, GSRT_FLAG_STATS, GSRT_FLAG_OUT_DUMP8 or a sharded entry point */
    GSRT_FLAG_FEATURES = 0x1000, /* whole COR frames: blend the scene's feature table instead of colour
                                   (gsrt_render_features below); GSRT_E_ARG with REF, GSRT_FLAG_STATS, GSRT_FLAG_OUT_DUMP8,
                                   GSRT_FLAG_DEPTH or a sharded entry point; GSRT_E_STATE without a feature table */
    GSRT_FLAG_FEATURE_GRAD = 0x2000, /* whole COR frames: the backward of a feature frame to the feature table; set by
                                       gsrt_render_feature_grad (below) itself, GSRT_E_ARG through every other entry point */
    GSRT_FLAG_SH_GRAD = 0x4000, /* whole COR frames: the backward of a colour frame to the SH table; set by gsrt_render_sh_grad
                                   (below) itself, GSRT_E_ARG through every other entry point */
    GSRT_FLAG_OPACITY_GRAD = 0x8000, /* whole COR frames: the backward of a colour frame to the opacities; set by
                                       gsrt_render_opacity_grad (below) itself, GSRT_E_ARG through every other entry point */
    GSRT_FLAG_SPLAT_GRAD = 0x20000, /* whole COR frames: the backward of a colour frame to each Gaussian's screen-space
                                      centre and conic; set by gsrt_render_splat_grad (below) itself, GSRT_E_ARG through
                                      every other entry point and with GSRT_FLAG_LUT (0x10000 is no flag: "bad mode") */
    GSRT_FLAG_SPLAT_DEPTH_GRAD = 0x80000 /* whole COR frames: the backward of a depth frame (RGBA and depth image) to the
                                            splat rows; set by gsrt_render_splat_depth_grad (below) itself, GSRT_E_ARG
                                            through every other entry point and with GSRT_FLAG_LUT (0x40000, like
                                            0x10000, is no flag: "bad mode") */
};
/* synthetic cloud kinds */
enum { GSRT_SYNTH_COR = 0, GSRT_SYNTH_REF = 1, GSRT_SYNTH_NEEDLE = 2 };

const char* gsrt_status_string(gsrt_status s);
int gsrt_abi_version(void);

/* ---- context ------------------------------------------------------------------------------ */
/* device_ordinal >= 0: HIP device. Fails with GSRT_E_DEVICE when the device is absent. */
gsrt_status gsrt_create(gsrt_ctx** out, int device_ordinal);
void gsrt_destroy(gsrt_ctx* ctx);
const char* gsrt_last_error(const gsrt_ctx* ctx);
gsrt_status gsrt_synchronize(gsrt_ctx* ctx);
/* the HIP stream the render kernels of this ctx are enqueued on (hipStream_t), for callers timing with
 * events; gsrt_synchronize() also reports (and clears) a traversal failure of any frame since the last
 * check (GSRT_E_DEVICE) */
void* gsrt_stream(gsrt_ctx* ctx);
/* the HIP stream of the per-frame prep kernels and of scene updates / refits (hipStream_t). It can change
 * between frames: a COR frame may move the prep work to a stream of another priority class (ordered after
 * everything queued on the previous one), so query it right before each use */
void* gsrt_prep_stream(gsrt_ctx* ctx);
/* the HIP stream (hipStream_t) of gsrt_scene_update's and gsrt_refit_bvh's copies (created at the first call): a producer
 * on the GPU fills an update's device source on this stream before the call. The copies go into the array's second
 * buffer and overlap the frames already queued ("Scene updates") */
void* gsrt_update_stream(gsrt_ctx* ctx);
/* 1 when the last frame ran on slot streams: its prep and render kernels on its frame slot's stream, overlapping
 * the previous frame (chosen per frame from sampled render kernel times), else 0 */
int gsrt_slot_streams(const gsrt_ctx* ctx);

/* ---- scene (replaces Assets::Scene, Scene.cpp:16-182) -------------------------------------- */
/* params/aabbs as the reference packs them (one entry per Gaussian model); sh nullable, n*48 floats
 * laid out [gauss][coef 0..15][rgb]. Host pointers; copied to HBM. */
gsrt_status gsrt_scene_from_params(gsrt_ctx* ctx, const gsrt_gauss_param* params, const gsrt_aabb* aabbs,
                                   uint32_t n, const float* sh, gsrt_scene** out);
/* Model::CreateGauss + Gauss::init_cov3d/init_radius (Model.cpp:550-564, Sphere.hpp:108-165), computed
 * on the device. rot_rxyz is the reference's vec4(r, x, y, z). Each of the five arrays is a host or a device pointer, on
 * its own (a device sh is transposed on the device, as gsrt_scene_set_sh does): a model that lives on the device, such as
 * gsrt_densify's output, becomes a scene without a host round trip. A device source must hold its data when the call
 * is made; the call returns when it has been read. */
gsrt_status gsrt_scene_from_model(gsrt_ctx* ctx, const float* center, const float* rot_rxyz, const float* scale,
                                  const float* opacity, const float* sh, uint32_t n, gsrt_scene** out);
/* download the device-side GaussParam / AABB arrays (either may be NULL) */
gsrt_status gsrt_scene_download(gsrt_scene* scene, gsrt_gauss_param* params, gsrt_aabb* aabbs);
uint32_t gsrt_scene_size(const gsrt_scene* scene);
void gsrt_destroy_scene(gsrt_scene* scene);
/* Per-Gaussian feature channels for feature frames (GSRT_FLAG_FEATURES, gsrt_render_features). feat: n*channels floats
 * laid out [gauss][channel], a host or device pointer, copied (into one 64-byte row per Gaussian); 1 <= channels <=
 * GSRT_MAX_FEATURES. feat == NULL with channels == 0 removes the table; channels == 0 with data, or above
 * GSRT_MAX_FEATURES, is GSRT_E_ARG. The call first waits for every queued frame of the context, then replaces the table.
 * Features are indexed by Gaussian id: gsrt_scene_update, gsrt_scene_attach, gsrt_scene_stream_pages and refits leave
 * them as they are. gsrt_scene_features: the channel count, 0 when the scene has no table. */
#define GSRT_MAX_FEATURES 16u
gsrt_status gsrt_scene_set_features(gsrt_scene* scene, const float* feat, uint32_t channels);
uint32_t gsrt_scene_features(const gsrt_scene* scene);
/* Replace the scene's SH rows. sh: n*48 floats laid out [gauss][coef 0..15][rgb] as at creation, a host or device pointer,
 * copied (a device source is transposed on the device, without a host round trip); sh == NULL removes the rows, and the
 * scene then renders colour 1. The call first waits for every queued frame of the context. A frame after it is byte for
 * byte the frame of a scene created with the same sh. */
gsrt_status gsrt_scene_set_sh(gsrt_scene* scene, const float* sh);

/* 3DGS .ply ingestion (the reference only has hard-coded CreateGauss calls,
 * SceneList.cpp:123-125). Vertex properties x y z, scale_0..2 (log), rot_0..3 (w x y z, unnormalised),
 * opacity (logit), f_dc_0..2 and f_rest_* (channel-major); ascii or binary, any scalar type.
 * gsrt_ply_info: vertex count and SH degree (0 when only f_dc or none). gsrt_ply_read: arrays in the
 * gsrt_scene_from_model convention (scale = exp, opacity = sigmoid, rot normalised (r,x,y,z), sh
 * [gauss][coef 0..15][rgb], nullable, degree cut or zero-padded to 3). */
gsrt_status gsrt_ply_info(const char* path, uint32_t* n, uint32_t* sh_degree);
gsrt_status gsrt_ply_read(const char* path, float* center, float* rot_rxyz, float* scale, float* opacity, float* sh);
gsrt_status gsrt_scene_from_ply(gsrt_ctx* ctx, const char* path, int with_sh, gsrt_scene** out);
/* The writer: a binary little-endian 3DGS .ply of the raw model (gsrt_model_arrays below, host pointers: unnormalised
 * quaternion, log scale, logit; what gsrt_model_deactivate gives and gsrt_model_step optimises), every value written as
 * the float32 it is: nothing is recomputed. Properties, in 3DGS's order: x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity
 * scale_0..2 rot_0..3; the normals are 0, f_rest is channel-major (f_rest_(15 ch + j) = sh[1 + j][ch], the inverse of
 * the reader's permutation). raw->sh == NULL writes no f_dc and no f_rest properties. n may be 0.
 * GSRT_E_ARG: a NULL path, raw or required array (n > 0); a model with features. GSRT_E_IO: the file cannot be written. */
struct gsrt_model_arrays;
gsrt_status gsrt_ply_write(const char* path, uint32_t n, const struct gsrt_model_arrays* raw);

/* ---- triangle meshes co-traced with the Gaussians ---------------------- */
/* Scene 33 holds a triangle-mesh sphere beside its two Gaussians (SceneList.cpp:123, Model::CreateSphere,
 * isProcedural = false). A triangle hit takes part in the REF frame the way vulkan-sim orders it:
 *   - the closest triangle hit t_tri (Moller-Trumbore in the object space of the identity instance,
 *     vulkan_ray_tracing.cc:1184-1206, accepted when Tmin <= t/|d| <= Tmax, :925-931) becomes the
 *     traversal's min_thit;
 *   - Gaussian AABBs entered at or beyond it are culled (:806-807; gsrt restates the order-independent
 *     case: the mesh instance is traversed first);
 *   - a Gaussian report is accepted only when its depth < t_tri (instructions.cc:7050);
 *   - a round whose closest hit is the triangle runs RayTracing.rchit, whose Scatter() sets the payload's
 *     Trans to 0 (Scatter.glsl:14-70).
 * COR frames do not trace meshes (gsrt_render returns GSRT_E_ARG for a COR frame of a scene with a mesh). */
/* append an indexed triangle mesh (world coordinates, identity instance transform, Application.cpp:361-362);
 * vertices: nv*3 floats, indices: nt*3 u32 (< nv). Copied; the mesh BVH is rebuilt on the host and uploaded. */
gsrt_status gsrt_scene_add_mesh(gsrt_scene* scene, const float* vertices, uint32_t nv, const uint32_t* indices,
                                uint32_t nt);
uint32_t gsrt_scene_mesh_triangles(const gsrt_scene* scene);
/* Model::CreateSphere(center, radius) geometry (Model.cpp:566-629): 32 slices x 16 stacks,
 * GSRT_SPHERE_VERTICES positions (3 floats each) and GSRT_SPHERE_TRIANGLES triangles (3 u32 each) */
#define GSRT_SPHERE_VERTICES 561u
#define GSRT_SPHERE_TRIANGLES 1024u
gsrt_status gsrt_sphere_mesh(const float center[3], float radius, float* vertices, uint32_t* indices);

/* ---- camera (replaces RayTracer::GetUniformBufferObject, RayTracer.cpp:38-65) --------------- */
/* mv: initial camera modelview (CameraInitialSate::ModelView), run through ModelViewController. */
gsrt_status gsrt_camera_from_modelview(const float mv[16], float fovy_deg, uint32_t width, uint32_t height,
                                       float focus_distance, uint32_t samples, uint32_t bounces, gsrt_ubo* out);
/* .camera file: 6 floats eye, centre -> lookAt(eye, centre, (0,1,0)) (SceneList.cpp:705-712) */
gsrt_status gsrt_camera_from_file(const char* path, float fovy_deg, uint32_t width, uint32_t height,
                                  float focus_distance, uint32_t samples, uint32_t bounces, gsrt_ubo* out);
gsrt_status gsrt_lookat(const float eye[3], const float center[3], const float up[3], float out_mv[16]);

/* ---- acceleration structure (replaces the Embree TLAS build, lvp_acceleration_structure.c:1329-1351) */
/* LBVH on the device: Morton codes, LSD radix sort, Karras hierarchy, bottom-up AABB fit. */
gsrt_status gsrt_build_bvh(gsrt_scene* scene);
/* new AABBs (host or device pointer, n entries; NULL = the scene's current AABBs) with the topology
 * kept: a bottom-up refit without a host round trip (one-wave workgroups fit 256-leaf chunks in LDS, then spans
 * of 16K and 1M leaves and the top climb by arrival counts). The copy is enqueued on gsrt_update_stream() into the
 * array's second buffer, ordered after the frames that read that buffer; frames queued after the call read the new
 * AABBs. The fit itself runs lazily with the next frame that uses a frame slot (a REF or counting frame, or a BVH
 * download, also refits a slot whose leaf boxes a COR frame replaced by footprint boxes; a rank of a sharded frame
 * fits only the part of the tree its band can see). A device source must hold its data when the call is made
 * (filled synchronously, or on gsrt_update_stream()) and stay unchanged until gsrt_synchronize(). The
 * reference only builds (MODE_BUILD, TopLevelAccelerationStructure.cpp:34); refit serves dynamic
 * scenes. */
gsrt_status gsrt_refit_bvh(gsrt_scene* scene, const gsrt_aabb* aabbs);
/* replace the scene's GaussParam and/or AABB arrays (host or device pointers, n entries each, either may be NULL),
 * with the same stream, ordering and source rules as gsrt_refit_bvh (a producer on the GPU fills the source on
 * gsrt_update_stream()); follow with gsrt_refit_bvh(scene, NULL) when AABBs moved. The animation step of a dynamic scene
 * (config 5: per-frame centre jitter). */
gsrt_status gsrt_scene_update(gsrt_scene* scene, const gsrt_gauss_param* params, const gsrt_aabb* aabbs);
/* the zero-copy form of gsrt_scene_update for a producer that writes each frame's Gaussians into device arrays of its
 * own: frames queued from now on read params / aabbs (device pointers on the context's device, 16-byte aligned,
 * n entries; either may be NULL = unchanged) in place. The arrays must hold their data at the call (filled
 * synchronously or on gsrt_update_stream()) and stay unchanged and allocated until gsrt_scene_detach() or
 * gsrt_destroy_scene() returns; attaching again swaps in other arrays under the same rule. Follow with
 * gsrt_refit_bvh(scene, NULL) when AABBs moved. A gsrt_scene_update / gsrt_refit_bvh source for an attached array, or
 * gsrt_scene_stream_pages, copies into the scene's own buffers and ends that borrow (the caller's array is then read
 * until gsrt_synchronize()). */
gsrt_status gsrt_scene_attach(gsrt_scene* scene, const gsrt_gauss_param* params, const gsrt_aabb* aabbs);
/* end a borrow: copy the attached arrays into the scene's own buffers and wait for every queued frame, so nothing
 * reads the caller's arrays after it returns */
gsrt_status gsrt_scene_detach(gsrt_scene* scene);
/* Gaussian pages: a dynamic scene whose Gaussians change on the host streams
 * them into HBM page by page. Page p holds Gaussians [p * GSRT_PAGE_GAUSSIANS, min((p + 1) * GSRT_PAGE_GAUSSIANS, n)).
 * gsrt_scene_stream_pages copies the listed pages of the full-scene host arrays params / aabbs (either may be NULL)
 * into the scene, consecutive page ids as one transfer, on gsrt_prep_stream() with gsrt_scene_update's ordering
 * (after every queued frame that reads the arrays, before the next frame's prep); follow with
 * gsrt_refit_bvh(scene, NULL) when AABBs moved. The copies run on the DMA engines beside the render kernels and
 * return at once when the host arrays are page-locked (gsrt_host_register); the arrays must stay unchanged until
 * gsrt_synchronize(). pages: ascending or not, duplicates allowed, each < the page count. */
#define GSRT_PAGE_GAUSSIANS 4096u
gsrt_status gsrt_scene_stream_pages(gsrt_scene* scene, const gsrt_gauss_param* params, const gsrt_aabb* aabbs,
                                    const uint32_t* pages, uint32_t npages);
uint32_t gsrt_scene_pages(const gsrt_scene* scene);
/* page-lock (and unlock) caller memory for asynchronous streaming (hipHostRegister) */
gsrt_status gsrt_host_register(gsrt_ctx* ctx, void* ptr, size_t bytes);
gsrt_status gsrt_host_unregister(gsrt_ctx* ctx, void* ptr);
/* BVH introspection for tests: internal-node count, root box (6 floats), max depth */
gsrt_status gsrt_bvh_info(gsrt_scene* scene, uint32_t* n_internal, float root_box[6], uint32_t* max_depth);
/* raw node download for tests: nodes = (n-1)*16 u32/f32 words; leaf_gid = n u32 (sorted order) */
gsrt_status gsrt_bvh_download(gsrt_scene* scene, uint32_t* nodes, uint32_t* leaf_gid, uint32_t* morton_sorted);

/* ---- render (replaces vkCmdTraceRaysKHR(W,H,1) over GaussTracing.rgen, Application.cpp:223-225) */
/* mode: GSRT_MODE_* | flags. k: 0 = mode default (REF: 8, the reference's NextK width; COR: the
 * tile-shared nearest-hit buffer capacity). rgba_out: W*H*4 floats (RGBA32F, row-major), host or
 * device pointer, may be NULL (image stays in the ctx framebuffer). raystate_out: W*H entries, host
 * or device pointer, nullable. Blocks until the frame is done when any output is a host pointer.
 * The traversal error word is sticky across pipelined frames: a synchronous render (gsrt_render,
 * gsrt_render_sharded) that drains the ctx reports and clears a failure of
 * any earlier gsrt_render_async frame as well (GSRT_E_DEVICE), exactly as gsrt_synchronize does. */
gsrt_status gsrt_render(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* rgba_out,
                        gsrt_raystate* raystate_out);
/* enqueue one frame on gsrt_stream(); outputs (device pointers only) may be NULL */
gsrt_status gsrt_render_async(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* d_rgba,
                              gsrt_raystate* d_raystate);
/* device pointer of the ctx framebuffer of the last render (W*H*4 floats). Frames on slot streams
 * (gsrt_slot_streams) alternate between two buffers, so query it after each render rather than keeping it. NULL after
 * a GSRT_FLAG_OUT_DUMP8 sharded frame (its image is read with gsrt_dump8_read), until the next RGBA32F frame */
const float* gsrt_framebuffer(gsrt_ctx* ctx);
/* Expected depth of a COR frame (GSRT_FLAG_DEPTH). Per sample ray, over exactly the hits the colour blend takes (the same
 * order, the same alpha, the same stop before a hit that would take T below 1e-4):
 *     D = sum_i z_i w_i,   w_i = alpha_i T_i (the blend's own weight), accumulated front to back as fma(z_i, w_i, D),
 * and a pixel's depth combines its samples' D exactly as its colour channels are combined. z_i is the float32 view depth
 * of Gaussian i's centre (the key the hits are sorted by): the convention of rasterised 3DGS, not the point of maximum
 * response along the ray. The value is premultiplied, like the colour: divide by rgba[3] for a normalised depth; a
 * pixel that blends nothing holds 0. depth: W*H floats, row-major. The frame's RGBA is the plain frame's, bit for bit.
 * A depth frame always takes the in-order path: one depth image per ctx, frames in stream order on gsrt_stream(), never
 * on slot streams (gsrt_slot_streams reads 0 after it); plain frames before and after it choose as they do without it.
 * Not provided: depth of sharded frames, depth on slot streams, median or nearest-hit depth, a normalised output.
 * gsrt_render_depth sets the flag itself; rgba_out / depth_out are host or device pointers, either may be NULL (the
 * images stay in gsrt_framebuffer / gsrt_depth_buffer); it blocks until the frame is done, like gsrt_render.
 * gsrt_render / gsrt_render_async with the flag render the same frame and leave the depth in gsrt_depth_buffer. */
gsrt_status gsrt_render_depth(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* rgba_out,
                              float* depth_out);
/* the same, enqueued on gsrt_stream(); outputs (device pointers only) may be NULL */
gsrt_status gsrt_render_depth_async(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* d_rgba,
                                    float* d_depth);
/* device pointer of the last frame's depth image (W*H floats), or NULL when the last frame had none */
const float* gsrt_depth_buffer(gsrt_ctx* ctx);
/* Feature frame (GSRT_FLAG_FEATURES): a whole COR frame that blends the scene's feature table (gsrt_scene_set_features,
 * C channels) with the renderer's own weights. Per sample ray and channel c, over exactly the hits the colour blend takes
 * (the same candidates and order, the same alpha with its min(., 0.99) and lower cut, the same stop before a hit that
 * would take T below 1e-4):
 *     F_c = sum_i f_{g_i,c} w_i,   w_i = alpha_i T_i, accumulated front to back as fma(f, w_i, F_c) from +0,
 * and a pixel's F_c combines its samples' exactly as its colour channels and depth are combined. No clamp, no offset, no
 * normalisation: the values are premultiplied, negative and non-finite features pass through as IEEE arithmetic gives
 * them, a pixel that blends nothing holds +0 in every channel. feat: W*H*C floats, row-major, pixel-interleaved.
 * The frame's RGBA is that of the same geometry rendered without SH rows (colour 1), bit for bit, whether or not the
 * scene has SH rows: r = g = b = sum w (the normaliser), a = 1 - T; a feature frame evaluates no SH.
 * Like a depth frame, a feature frame always takes the in-order path: one feature image per ctx, frames in stream order
 * on gsrt_stream(), never on slot streams (gsrt_slot_streams reads 0 after it); plain frames before and after it choose
 * as they do without it. GSRT_E_STATE when the scene has no feature table.
 * Not provided: more than GSRT_MAX_FEATURES channels, features of sharded frames or on slot streams, colour in the same
 * frame, a normalised output.
 * gsrt_render_features sets the flag itself; rgba_out / feat_out are host or device pointers, either may be NULL (the
 * images stay in gsrt_framebuffer / gsrt_feature_buffer); it blocks until the frame is done, like gsrt_render.
 * gsrt_render / gsrt_render_async with the flag render the same frame and leave the image in gsrt_feature_buffer. */
gsrt_status gsrt_render_features(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* rgba_out,
                                 float* feat_out);
/* the same, enqueued on gsrt_stream(); outputs (device pointers only) may be NULL */
gsrt_status gsrt_render_features_async(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, float* d_rgba,
                                       float* d_feat);
/* device pointer of the last frame's feature image (W*H*C floats), or NULL when the last frame had none (after a feature
 * frame gsrt_depth_buffer reads NULL, after a depth frame this does) */
const float* gsrt_feature_buffer(gsrt_ctx* ctx);
/* Gradient frame (GSRT_FLAG_FEATURE_GRAD): the exact backward of a feature frame with respect to the feature table,
 * which the frame is linear in. grad_image is the upstream gradient G of a feature image, W*H*channels floats laid out as
 * that image is (row-major, pixel-interleaved); grad_table receives n*channels floats laid out [gauss][channel]:
 *     grad_table[g][c] = sum over pixels p, samples s of p, hits i of ray (p, s) with id g of   w_i * (G[p][c] / ns)
 * with ns the samples per pixel and the hits, their order, alpha and the stop exactly those of the feature frame's blend.
 * Each term is the float32 product of the blend's own float32 weight w_i and G[p][c] / ns (G * (1/ns) when ns is a power
 * of two, G / ns otherwise, rounded once). The terms are summed on the device with float atomic adds, so the order of the
 * sum is unspecified and results can differ in their last bits from run to run. A non-finite G[p][c] reaches only the
 * Gaussians pixel p blends. No feature table is needed or read; 1 <= channels <= GSRT_MAX_FEATURES.
 * accumulate == 0: the table is written, Gaussians no ray blends get +0. accumulate != 0: this frame's gradient is added
 * to what the table holds (batches of views); that form takes a device grad_table only, a host one is GSRT_E_ARG.
 * grad_image / grad_table are host or device pointers. A device table must be ordinary device memory (hipMalloc, a torch
 * tensor); host tables go through a buffer of the ctx.
 * With channels == 1 and G == 1 everywhere the result is each Gaussian's blend weight summed over the frame's pixels
 * (the mean over a pixel's samples): its contribution to the view, the importance score used for pruning.
 * The frame's RGBA (gsrt_framebuffer) is the feature frame's (r = g = b = sum w, a = 1 - T). Like depth and feature frames
 * it takes the in-order path on gsrt_stream(): gsrt_slot_streams reads 0 after it, gsrt_depth_buffer and
 * gsrt_feature_buffer read NULL; gsrt_timing records the frame like any other.
 * GSRT_E_ARG (gsrt_last_error names GSRT_FLAG_FEATURE_GRAD, and the context renders as before): REF mode; GSRT_FLAG_STATS,
 * GSRT_FLAG_OUT_DUMP8, GSRT_FLAG_DEPTH or GSRT_FLAG_FEATURES with it; sharded entry points; a scene with a mesh; channels
 * out of range; a NULL grad_image or grad_table; the flag passed to gsrt_render / gsrt_render_async (or the depth and
 * feature forms), which have nowhere to take the image.
 * Not provided: gradients with respect to geometry or the normaliser (sum w); sharded frames; more than
 * GSRT_MAX_FEATURES channels.
 * gsrt_render_feature_grad blocks until the table is complete, like gsrt_render. */
gsrt_status gsrt_render_feature_grad(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                     const float* grad_image, uint32_t channels, float* grad_table, int accumulate);
/* the same, enqueued on gsrt_stream(); device pointers only */
gsrt_status gsrt_render_feature_grad_async(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                           const float* d_grad_image, uint32_t channels, float* d_grad_table,
                                           int accumulate);
/* SH gradient frame (GSRT_FLAG_SH_GRAD): the backward of a plain COR colour frame with respect to the scene's SH table.
 * Apart from the clamp at 0 the colour is linear in the coefficients, so the backward is one forward-ordered pass.
 * grad_image is the upstream gradient G of the RGBA frame, W*H*4 floats laid out as the frame is; channel 3 is ignored
 * (alpha does not depend on SH). grad_table receives n*48 floats laid out [gauss][coef 0..15][rgb], as the sh of
 * gsrt_scene_from_params is:
 *     grad_table[g][q][ch] = sum over pixels p, samples s of p, hits i of ray (p, s) with id g and a_{i,ch} > 0 of
 *                            w_i * Y_q(d_{p,s}) * (G[p][ch] / ns)
 * with ns the samples per pixel; w_i, the hits, their order and the stop exactly those of the colour blend; a_{i,ch} the
 * blend's own float32 channel value before its clamp at 0; Y_q the ray's float32 SH basis (Y_0 = 0.28209479: the gradient
 * is with respect to s_0 as the API takes it). The clamp's mask is a select: a clamped channel contributes +0, and a
 * non-finite G[p][ch] reaches only the (Gaussian, channel) pairs pixel p blends unclamped. G / ns is formed once (G * (1/ns)
 * for a power of two, G / ns otherwise); a term is the float32 product (w_i * that) * Y_q. The terms are summed on the
 * device with float atomic adds, so the order of the sum is unspecified and results can differ in their last bits from
 * run to run.
 * accumulate == 0: the table is written, entries nothing reaches get +0. accumulate != 0: this frame's gradient is added
 * to what the table holds; that form takes a device grad_table only, a host one is GSRT_E_ARG. grad_image / grad_table are
 * host or device pointers; a device table must be ordinary device memory.
 * The frame's RGBA (gsrt_framebuffer) is the plain colour frame's, bit for bit. Like depth, feature and feature-gradient
 * frames it takes the in-order path on gsrt_stream(): gsrt_slot_streams reads 0 after it, gsrt_depth_buffer and
 * gsrt_feature_buffer read NULL; gsrt_timing records the frame like any other.
 * GSRT_E_STATE: a scene without SH rows. GSRT_E_ARG (gsrt_last_error names GSRT_FLAG_SH_GRAD, and the context renders as
 * before): REF mode; GSRT_FLAG_STATS, GSRT_FLAG_OUT_DUMP8, GSRT_FLAG_DEPTH, GSRT_FLAG_FEATURES or GSRT_FLAG_FEATURE_GRAD with
 * it; sharded entry points; a scene with a mesh; a NULL grad_image or grad_table; the flag passed to any other entry point.
 * Not provided: gradients with respect to geometry (opacity: gsrt_render_opacity_grad below); sharded frames.
 * gsrt_render_sh_grad blocks until the table is complete, like gsrt_render. */
gsrt_status gsrt_render_sh_grad(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k, const float* grad_image,
                                float* grad_table, int accumulate);
/* the same, enqueued on gsrt_stream(); device pointers only */
gsrt_status gsrt_render_sh_grad_async(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                      const float* d_grad_image, float* d_grad_table, int accumulate);
/* Opacity gradient frame (GSRT_FLAG_OPACITY_GRAD): the backward of a plain COR colour frame (RGBA) with respect to each
 * Gaussian's opacity, gsrt_gauss_param::center_opacity[3], i.e. the opacity of gsrt_scene_from_model. The blend is ordered
 * front to back, so every ray is shaded twice in the same order: once for its final colour and transmittance, then again,
 * where the colour behind a hit is the final colour minus the running colour.
 * grad_image is the upstream gradient G of the RGBA frame, W*H*4 floats laid out as the frame is; all four channels are
 * used (alpha depends on opacity). grad_table receives n floats, [gauss].
 * For sample ray (p, s) with blended hits i = 1..N in the blend's order, with the blend's own alpha_i, T_i (the
 * transmittance before hit i) and w_i = alpha_i T_i, col_{i,ch} the clamped SH colour the blend used (1 without SH rows),
 * the ray's finals C_ch = sum_i col_{i,ch} w_i and T_end = T_{N+1}:
 *     Cafter_{i,ch} = the blend's running colour after hit i (fma(col, w, C))
 *     d_i  = sum_ch Gs[ch] * (T_i col_{i,ch} - (C_ch - Cafter_{i,ch}) / (1 - alpha_i))  +  Gs[3] * T_end / (1 - alpha_i)
 *     grad_table[g] = sum over p, s, hits i with id g and fl(|o_g| e_i) < 0.99f of   d_i * e_i
 * Gs = G[p] / ns, formed once (G * (1/ns) for a power of two, G / ns otherwise); e_i is the blend's own float32
 * exponential, or the LUT's value under GSRT_FLAG_LUT; the division is one float32 reciprocal of 1 - alpha_i per hit. A hit
 * whose alpha was clamped to 0.99 contributes +0; that is a select, so a non-finite G[p] reaches only the Gaussians pixel p
 * blends unclamped. Sets fixed by the forward frame and not differentiated: the hits taken and their order, the
 * alpha > 1/255 cut and gcut, and the stop before a hit that would take T below 1e-4. The terms are summed on the device
 * with float atomic adds, so the order of the sum is unspecified and results can differ in their last bits from run to run.
 * accumulate == 0: the table is written, entries nothing reaches get +0. accumulate != 0: this frame's gradient is added
 * to what the table holds; that form takes a device grad_table only, a host one is GSRT_E_ARG. grad_image / grad_table are
 * host or device pointers; a device table must be ordinary device memory.
 * The frame's RGBA (gsrt_framebuffer) is the plain colour frame's, bit for bit. Like the other gradient frames it takes the
 * in-order path on gsrt_stream(): gsrt_slot_streams reads 0 after it, gsrt_depth_buffer and gsrt_feature_buffer read NULL;
 * gsrt_timing records the frame like any other. Scenes with and without SH rows are both served.
 * GSRT_E_ARG (gsrt_last_error names GSRT_FLAG_OPACITY_GRAD, and the context renders as before): REF mode; GSRT_FLAG_STATS,
 * GSRT_FLAG_OUT_DUMP8, GSRT_FLAG_DEPTH, GSRT_FLAG_FEATURES, GSRT_FLAG_FEATURE_GRAD or GSRT_FLAG_SH_GRAD with it; sharded entry
 * points; a scene with a mesh; a NULL grad_image or grad_table; the flag passed to any other entry point.
 * Not provided here: gradients with respect to means and covariances (gsrt_render_splat_grad) or SH
 * (gsrt_render_sh_grad); sharded frames.
 * gsrt_render_opacity_grad blocks until the table is complete, like gsrt_render. */
gsrt_status gsrt_render_opacity_grad(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                     const float* grad_image, float* grad_table, int accumulate);
/* the same, enqueued on gsrt_stream(); device pointers only */
gsrt_status gsrt_render_opacity_grad_async(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                           const float* d_grad_image, float* d_grad_table, int accumulate);
/* Splat gradient frame (GSRT_FLAG_SPLAT_GRAD): the backward of a plain COR colour frame (RGBA) with respect to what the
 * projection gives each Gaussian on the screen: the pixel centre (ppx, ppy) and the conic (A, B, C) of
 * g = (A dx^2 + 2 B dx dy + C dy^2) / 2, dx = px - ppx, dy = py - ppy for a ray through pixel coordinate (px, py). It is
 * the view-space gradient that densification thresholds on, and gsrt_splat_grad_to_model (below) chains it to the
 * Gaussians' centres and covariances. Every ray is shaded twice, as for gsrt_render_opacity_grad.
 * grad_image is the upstream gradient G of the RGBA frame, W*H*4 floats, all four channels used. grad_splat receives n
 * rows of 8 floats (32 bytes), [gauss][slot].
 * With alpha_i, T_i, col_i, the finals, Gs and d_i exactly as gsrt_render_opacity_grad defines them, dx and dy the float32
 * differences the forward forms and e_i its float32 exponential: for every blended hit i of Gaussian g whose
 * fl(|o_g| e_i) < 0.99f, with q_i = -alpha_i d_i (d alpha / dg = -alpha where the clamp let o e through),
 *     row[0] += q_i * -(A dx + B dy)     dL/dppx          row[3] += q_i * dx dy            dL/dB
 *     row[1] += q_i * -(B dx + C dy)     dL/dppy          row[4] += q_i * dy^2 / 2         dL/dC
 *     row[2] += q_i * dx^2 / 2           dL/dA            row[5] += d_i * e_i              dL/d opacity
 * and row[6] = row[7] = +0. Slot 5 is the sum gsrt_render_opacity_grad defines: one backward frame serves geometry and
 * opacity. A hit whose alpha was clamped to 0.99 contributes +0 to every slot (a select). Sets fixed by the forward
 * frame and not differentiated: the hits taken and their order (the depth key), the AABB slab test, the alpha > 1/255 cut
 * and gcut, and the stop. The colour does not depend on the geometry: the SH basis is the ray's. The terms are summed
 * with float atomic adds: the order of a sum is unspecified.
 * accumulate, host and device pointers, the framebuffer (the plain colour frame's, bit for bit), the in-order path and
 * timing: as for gsrt_render_opacity_grad; with accumulate != 0 slots 6 and 7 keep what they hold. Scenes with and without
 * SH rows are both served.
 * GSRT_E_ARG (gsrt_last_error names GSRT_FLAG_SPLAT_GRAD, and the context renders as before): REF mode; GSRT_FLAG_LUT
 * (under the LUT the exponential is piecewise linear and d alpha / dg is a segment's slope, not -alpha); GSRT_FLAG_STATS,
 * GSRT_FLAG_OUT_DUMP8, GSRT_FLAG_DEPTH, GSRT_FLAG_FEATURES or another gradient flag with it; sharded entry points; a scene
 * with a mesh; a NULL grad_image or grad_splat; the flag passed to any other entry point.
 * Not provided: LUT frames; sharded frames; gradients through the hit order, the AABB test or the stop; SH
 * (gsrt_render_sh_grad).
 * gsrt_render_splat_grad blocks until the table is complete, like gsrt_render. */
gsrt_status gsrt_render_splat_grad(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                   const float* grad_image, float* grad_splat, int accumulate);
/* the same, enqueued on gsrt_stream(); device pointers only */
gsrt_status gsrt_render_splat_grad_async(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                         const float* d_grad_image, float* d_grad_splat, int accumulate);
/* The COR projection backwards: the splat rows of gsrt_render_splat_grad (n x 8 floats; slots 0..4 are read) chained to
 * the gradients with respect to each Gaussian's centre, grad_center (n x 3 floats, center_opacity[0..3)), and its
 * covariance, grad_cov (n x 6 floats in cov3d's order xx, xy, xz, yy, yz, zz; an off-diagonal entry is one variable that
 * stands twice in Sigma, so its gradient is the sum of both places). ubo is the frame's; the scene's current parameters
 * are read, a borrowed array included (gsrt_scene_attach). One lane per Gaussian recomputes the projection's float32
 * intermediates: V = T Sigma T^T + 0.3 I with the 0.3 a constant, Q = V^-1, dL/dV = -Q [[dA, dB/2], [dB/2, dC]] Q; the
 * centre receives its part through (ppx, ppy), with the general projection matrix, and through T's dependence on the
 * view-space position. A Gaussian the projection marks invalid (depth <= 0 or det <= 0) gets +0, and with accumulate == 0
 * so does every entry that comes out as zero, those of a Gaussian whose row is all +0 (no ray reached it) among them.
 * Nothing flows through the depth key, the AABB or the footprint. No atomics: the result is deterministic.
 * accumulate == 0: both tables are written. accumulate != 0: added to; device tables only. All three tables are host or
 * device pointers (ordinary device memory), each on its own.
 * GSRT_E_ARG: a NULL pointer; a host table with accumulate; a scene with a mesh. GSRT_E_STATE: before gsrt_build_bvh, as
 * for a render. gsrt_splat_grad_to_model blocks until the tables are complete. */
gsrt_status gsrt_splat_grad_to_model(gsrt_scene* scene, const gsrt_ubo* ubo, const float* grad_splat, float* grad_center,
                                     float* grad_cov, int accumulate);
/* the same, enqueued on gsrt_stream(); device pointers only */
gsrt_status gsrt_splat_grad_to_model_async(gsrt_scene* scene, const gsrt_ubo* ubo, const float* d_grad_splat,
                                           float* d_grad_center, float* d_grad_cov, int accumulate);
/* Splat-depth gradient frame (GSRT_FLAG_SPLAT_DEPTH_GRAD): the backward of a depth frame (gsrt_render_depth: the RGBA frame
 * and the expected depth D = sum_i z_i w_i together) to the splat rows of gsrt_render_splat_grad, with the view depth's own
 * gradient in slot 6. Depth is one more blended channel whose colour is the hit's own z_i, and that colour has a gradient
 * of its own. Every ray is shaded twice, as for gsrt_render_splat_grad.
 * grad_image is the upstream gradient G of the RGBA frame, W*H*4 floats; grad_depth the upstream gradient Gdepth of the
 * depth image, W*H floats; Gs = G[p] / ns and Gd = Gdepth[p] / ns, each formed once (x * (1/ns) for a power of two, x / ns
 * otherwise). grad_splat receives n rows of 8 floats, [gauss][slot].
 * Per sample ray, over exactly the hits the colour blend takes (the same order, alpha and stop), with z_i the float32 view
 * depth the depth frame blends and the hits are keyed by, and everything else as gsrt_render_splat_grad names it:
 *     Dafter_i = fma(z_i, w_i, Dafter_{i-1}) from +0,  D = Dafter_N      (the depth frame's own arithmetic)
 *     d_i  = (gsrt_render_splat_grad's d_i)  +  Gd * (T_i z_i - (D - Dafter_i) * r),   r = 1 / (1 - alpha_i),
 * r the same single float32 reciprocal d_i's other terms are divided by. Slots 0..5 are gsrt_render_splat_grad's formulas
 * with this d_i; a hit whose alpha the clamp at 0.99 replaced contributes +0 to them (a select). Further
 *     row[6] += w_i * Gd                 dL/dz (the view depth, -t_2 of the centre's view-space position)
 * on every blended hit, clamped or not: dD/dz_i = w_i does not pass through the clamp. row[7] = +0. Not differentiated, as
 * for gsrt_render_splat_grad: the hits taken and their order (the depth key), the AABB slab test, the alpha > 1/255 cut
 * and gcut, and the stop. The terms are summed with float atomic adds: the order of a sum is unspecified.
 * accumulate, host and device pointers, the framebuffer (the plain colour frame's, bit for bit; gsrt_depth_buffer and
 * gsrt_feature_buffer read NULL), the in-order path (gsrt_slot_streams reads 0) and timing: as for
 * gsrt_render_splat_grad; with accumulate != 0 slot 7 keeps what it holds. Scenes with and without SH rows are served.
 * GSRT_E_ARG (gsrt_last_error names GSRT_FLAG_SPLAT_DEPTH_GRAD, and the context renders as before): REF mode;
 * GSRT_FLAG_LUT; GSRT_FLAG_STATS, GSRT_FLAG_OUT_DUMP8, GSRT_FLAG_DEPTH, GSRT_FLAG_FEATURES or another gradient flag with it;
 * sharded entry points; a scene with a mesh; a NULL grad_image, grad_depth or grad_splat; the flag passed to any other
 * entry point.
 * Not provided: LUT frames; sharded frames; gradients through the hit order; a normalised depth's backward (divide in the
 * caller: with a = rgba[3], d(D / a) takes Gdepth / a here and -Gdepth D / a^2 into G's alpha channel).
 * gsrt_render_splat_depth_grad blocks until the table is complete, like gsrt_render. */
gsrt_status gsrt_render_splat_depth_grad(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                         const float* grad_image, const float* grad_depth, float* grad_splat,
                                         int accumulate);
/* the same, enqueued on gsrt_stream(); device pointers only */
gsrt_status gsrt_render_splat_depth_grad_async(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                               const float* d_grad_image, const float* d_grad_depth, float* d_grad_splat,
                                               int accumulate);
/* gsrt_splat_grad_to_model for the rows of gsrt_render_splat_depth_grad: slots 0..4 and 6 are read. The view depth is
 * -t_2 with t = MV (c, 1), so slot 6 enters as dL/dt_2 -= row[6] before the final MV^T dL/dt; nothing of it flows to
 * grad_cov, which is gsrt_splat_grad_to_model's byte for byte. Same contract otherwise: invalid Gaussians get +0, no
 * atomics, accumulate with device tables only. */
gsrt_status gsrt_splat_depth_grad_to_model(gsrt_scene* scene, const gsrt_ubo* ubo, const float* grad_splat,
                                           float* grad_center, float* grad_cov, int accumulate);
/* the same, enqueued on gsrt_stream(); device pointers only */
gsrt_status gsrt_splat_depth_grad_to_model_async(gsrt_scene* scene, const gsrt_ubo* ubo, const float* d_grad_splat,
                                                 float* d_grad_center, float* d_grad_cov, int accumulate);
/* ---- adaptive density control: clone, split and prune a model on the device ----------------------
 * The model is the gsrt_scene_from_model arrays; the calls below work on arrays, not on a scene: a scene's size is fixed,
 * so after gsrt_densify the caller creates a new scene from the new arrays (gsrt_scene_from_model takes device pointers)
 * and builds its BVH. A split's samples come from the caller's noise, so a result is a pure function of its inputs;
 * gsrt_normal_noise (below) draws such noise on the device from a seed. 3DGS's screen-size prune is gsrt_view_stats_add
 * (the largest screen radius beside the statistic) with gsrt_densify_screen. Not provided: resizing a scene in place (an
 * opacity reset: gsrt_model_opacity_reset below), radii of sharded frames, a world-extent prune beyond max_scale. */
typedef struct gsrt_model_arrays {   /* the gsrt_scene_from_model convention */
    float* center;    /* n x 3 */
    float* rot_rxyz;  /* n x 4, used as given */
    float* scale;     /* n x 3 */
    float* opacity;   /* n */
    float* sh;        /* n x 48 [gauss][coef][rgb], nullable */
    float* features;  /* n x feature_channels, nullable */
    uint32_t feature_channels; /* 0..GSRT_MAX_FEATURES; 0 exactly when features is NULL */
} gsrt_model_arrays;

typedef struct gsrt_densify_params {
    float grad_threshold; /* densify when the mean view-space gradient norm is >= this */
    float split_scale;    /* a densified Gaussian whose largest scale is > this is split, otherwise cloned */
    float min_opacity;    /* prune unless opacity >= this (so a NaN opacity is pruned) */
    float max_scale;      /* prune when the largest scale is > this; <= 0 switches the test off */
    float shrink;         /* a split child's scales are the parent's / shrink (3DGS: 1.6); must be > 0 */
    uint32_t reserved[3]; /* zero, otherwise GSRT_E_ARG */
} gsrt_densify_params;

/* The densification statistic of one view, added to stats. grad_splat: the n rows of 8 floats of gsrt_render_splat_grad or
 * gsrt_render_splat_depth_grad for a frame of width x height pixels; stats: n x 2 floats [sum, count], which the caller
 * zeroes and this call always adds to. Per Gaussian g, in float32, in exactly this order:
 *     gx = row[0] * (0.5f * (float)width),  gy = row[1] * (0.5f * (float)height)
 *     norm = sqrtf(gx * gx + gy * gy)            (products and sum rounded one by one, a correctly rounded root)
 *     seen = any of row[0..5] != 0.0f            (a -0 is not seen, a NaN is)
 *     if seen: stats[g][0] += norm, stats[g][1] += 1; otherwise both words stay bit for bit as they were.
 * The scaling is that of 3DGS's viewspace_point_tensor.grad (the gradient with respect to the NDC position: a pixel is
 * 2 / width of NDC), so published thresholds such as 0.0002 carry over. "Seen" means that a ray's blend reached the
 * Gaussian with a gradient: the ray tracer's notion of visibility (a Gaussian behind an opaque one, or one no ray's
 * alpha cut lets through, is not seen), not the rasteriser's "inside the frustum". One lane per Gaussian and no atomics:
 * the result is deterministic.
 * grad_splat and stats are both host pointers or both device pointers (16-byte aligned rows on the device, as
 * hipMalloc and torch give them). The call runs on gsrt_stream(), behind the gradient frame that wrote the rows, and
 * blocks until stats is complete.
 * GSRT_E_ARG: a NULL ctx or pointer; one host and one device pointer; width or height 0; n > GSRT_MAX_GAUSSIANS. */
gsrt_status gsrt_density_stats_add(gsrt_ctx* ctx, uint32_t n, uint32_t width, uint32_t height, const float* grad_splat,
                                   float* stats);
/* the same, enqueued on gsrt_stream(); device pointers only */
gsrt_status gsrt_density_stats_add_async(gsrt_ctx* ctx, uint32_t n, uint32_t width, uint32_t height,
                                         const float* d_grad_splat, float* d_stats);
/* gsrt_densify's decision and row count alone: n_out = the rows gsrt_densify would write for these scales (n x 3),
 * opacities (n), stats (n x 2) and params, so that a caller can size the output arrays exactly. Each array is a host or a
 * device pointer, on its own. Blocks. GSRT_E_ARG: a NULL pointer (the arrays may be NULL when n is 0), bad params (a
 * non-zero reserved word, shrink not > 0), n > GSRT_MAX_GAUSSIANS. */
gsrt_status gsrt_densify_count(gsrt_ctx* ctx, uint32_t n, const float* scale, const float* opacity, const float* stats,
                               const gsrt_densify_params* params, uint32_t* n_out);
/* Clone, split, prune or keep every Gaussian of `in` (n of them) and write the new model to `out` in one ordered
 * compaction pass. Per Gaussian g, in float32:
 *     m     = the largest of the three scales (m = s0; if (s1 > m) m = s1; if (s2 > m) m = s2, as the scene build)
 *     mean  = stats[g][1] > 0 ? stats[g][0] / stats[g][1] : 0            (stats: gsrt_density_stats_add's)
 *     prune = !(opacity >= min_opacity) || (max_scale > 0 && m > max_scale)
 *     dens  = !prune && mean >= grad_threshold
 *     split = dens && m > split_scale,   clone = dens && !split
 * g takes c_g output rows: 0 when pruned, 1 when kept, 2 when cloned or split. Its rows start at o_g = the sum of c_h
 * over h < g: the output's order is the input's, and n_out = the sum of all c_g.
 *     keep:   row o_g is g, every field bit for bit;                       origin[o_g] = g
 *     clone:  rows o_g and o_g + 1 are both g, every field bit for bit;     origin = g, -1 - g
 *     split:  rows o_g + k, k = 0 and 1, are the children;                  origin = -1 - g for both
 * A split child k: z = noise[g][k][0..3], v_i = scale_i * z_i, x_j = (v_0 R[0][j] + v_1 R[1][j]) + v_2 R[2][j] with R the
 * rotation matrix of the scene build (row k, column j; its entries formed with the build's own expressions from rot_rxyz as
 * given), so that x has the covariance (S R)^T (S R) for unit normal z: the scene's own Sigma. centre'_j = centre_j + x_j,
 * scale'_i = scale_i / shrink; rotation, opacity, the SH row and the feature row are copied bit for bit. Every operation is
 * rounded on its own (no fused multiply-add), the division correctly.
 * noise: n x 2 x 3 floats of the caller's (standard normal draws for 3DGS's split); only a split Gaussian's are read.
 * origin: int32[cap]; a row holds g when it is Gaussian g itself (its optimiser state carries over) and -1 - g when it
 * was newly made from g (a fresh optimiser state).
 * cap: the rows `out` and origin have room for; 2 n always suffices. n_out is always written. When n_out > cap or
 * n_out > GSRT_MAX_GAUSSIANS nothing else is written: GSRT_E_ARG, and gsrt_last_error names the count needed.
 * in and out must agree on which of sh and features are present and on feature_channels; an out array that is the
 * matching in array is GSRT_E_ARG (the pass is not in place). All arrays (in, stats, noise, out, origin) are host pointers
 * or all are device pointers (sh on the device 16-byte aligned); n_out is a host pointer. The call runs on gsrt_stream()
 * and blocks until `out` is complete.
 * GSRT_E_ARG also: a NULL ctx, in, out, params or n_out; a NULL input array with n > 0 or output array with cap > 0; bad
 * params; feature_channels above GSRT_MAX_FEATURES or not matching features; n > GSRT_MAX_GAUSSIANS. */
gsrt_status gsrt_densify(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* stats, const float* noise,
                         const gsrt_densify_params* params, const gsrt_model_arrays* out, int32_t* origin, uint32_t cap,
                         uint32_t* n_out);
/* the same, enqueued on gsrt_stream() without a host synchronisation; device pointers only, d_n_out (one uint32)
 * included: when it reads more than cap (or than GSRT_MAX_GAUSSIANS) after the stream has run, nothing else was written,
 * which is for the caller to check. (A call for a larger n than any before it on this ctx allocates its workspace first.) */
gsrt_status gsrt_densify_async(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* d_stats,
                               const float* d_noise, const gsrt_densify_params* params, const gsrt_model_arrays* out,
                               int32_t* d_origin, uint32_t cap, uint32_t* d_n_out);
/* gsrt_density_stats_add for a scene's Gaussians (n is the scene's, width and height are the ubo's), and beside it 3DGS's
 * max_radii2D: the largest screen radius of each Gaussian over the views that saw it. One lane per Gaussian, no atomics.
 * stats (n x 2): exactly what gsrt_density_stats_add does for the same rows, bit for bit: the same operations in the same
 * order, the same "seen" rule; an unseen Gaussian's words are untouched.
 * radii (n floats, nullable; the caller zeroes it): only for a seen Gaussian whose COR projection of ubo is valid (its
 * centre in front of the camera, det V > 0), from the scene's current parameters (a borrowed array included, read as
 * gsrt_splat_grad_to_model reads it). With V = [[v00, v01], [v01, v11]] and det the COR projection's own float32 values
 * (V = T Sigma T^T + 0.3 I: the low-pass is included, as in 3DGS), in float32, each operation rounded on its own:
 *     mid  = 0.5f * (v00 + v11)
 *     disc = fmaf(mid, mid, -det)
 *     lam  = mid + sqrtf(fmaxf(0.1f, disc))
 *     r    = ceilf(3.0f * sqrtf(lam))
 *     if (r > radii[g]) radii[g] = r            (a NaN r stores nothing)
 * An unseen, behind-camera or singular Gaussian keeps its word bit for bit.
 * grad_splat, stats and radii are all host pointers or all device pointers (grad_splat 16-byte aligned on the device). The
 * call runs on gsrt_stream(), behind the gradient frame that wrote the rows, and blocks until both arrays are complete.
 * GSRT_E_ARG: a NULL scene, ubo, grad_splat or stats; mixed pointers; width or height 0; a scene with a triangle mesh.
 * GSRT_E_STATE: before gsrt_build_bvh. */
gsrt_status gsrt_view_stats_add(gsrt_scene* scene, const gsrt_ubo* ubo, const float* grad_splat, float* stats,
                                float* radii);
/* the same, enqueued on gsrt_stream(); device pointers only */
gsrt_status gsrt_view_stats_add_async(gsrt_scene* scene, const gsrt_ubo* ubo, const float* d_grad_splat, float* d_stats,
                                      float* d_radii);
/* gsrt_densify, gsrt_densify_async and gsrt_densify_count in every word of their contracts, with one more term in the
 * decision, 3DGS's screen-size prune (radii: gsrt_view_stats_add's, n floats, nullable):
 *     prune = prune || (radii && max_screen_radius > 0 && radii[g] > max_screen_radius)
 * A NaN radius does not prune. With radii == NULL or max_screen_radius <= 0 the result is gsrt_densify's, bit for bit (the
 * same kernels run). radii lives on the side, host or device, of the other arrays (on its own side for the count form).
 * GSRT_E_ARG also: a NaN max_screen_radius. 3DGS uses 20 pixels, after its first opacity reset. */
gsrt_status gsrt_densify_screen(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* stats,
                                const float* noise, const gsrt_densify_params* params, const float* radii,
                                float max_screen_radius, const gsrt_model_arrays* out, int32_t* origin, uint32_t cap,
                                uint32_t* n_out);
gsrt_status gsrt_densify_screen_async(gsrt_ctx* ctx, const gsrt_model_arrays* in, uint32_t n, const float* d_stats,
                                      const float* d_noise, const gsrt_densify_params* params, const float* d_radii,
                                      float max_screen_radius, const gsrt_model_arrays* out, int32_t* d_origin,
                                      uint32_t cap, uint32_t* d_n_out);
gsrt_status gsrt_densify_screen_count(gsrt_ctx* ctx, uint32_t n, const float* scale, const float* opacity,
                                      const float* stats, const gsrt_densify_params* params, const float* radii,
                                      float max_screen_radius, uint32_t* n_out);
/* Counter-based standard normal noise, e.g. gsrt_densify's: out[i], i < count, is a pure function of (seed, stream_id, i).
 * It does not depend on count or on how the work is laid out: a prefix of a longer call is the shorter call bit for bit.
 * The generator is Philox4x32-10 (Salmon et al. 2011, as Random123 states it) with the key (seed lo, seed hi); block j has
 * the counter (j lo, j hi, stream_id, 0), and its four output words x0..x3 give out[4j .. 4j + 3] as two Box-Muller pairs,
 * (x0, x1) -> out[4j], out[4j + 1] and (x2, x3) -> out[4j + 2], out[4j + 3]. Per pair (xa, xb), in float32, every operation
 * rounded on its own:
 *     ua = ((float)(xa >> 8) + 0.5f) * 2^-24,   ub = ((float)(xb >> 8) + 0.5f) * 2^-24        (both in (0, 1])
 *     r  = sqrtf(-2.0f * logf(ua)),   th = 6.2831855f * ub,   z0 = r * cosf(th),   z1 = r * sinf(th)
 * with the device's logf, cosf and sinf (accurate to a few ulp; |z| < 5.9). A count that is no multiple of 4 drops the
 * tail of the last block. out is a host or a device pointer (4-byte aligned; whole 16-byte stores are used where it is
 * 16-byte aligned); the call runs on gsrt_stream() and blocks until out is complete. count == 0 writes nothing.
 * GSRT_E_ARG: a NULL ctx, or a NULL or misaligned out with count > 0. */
gsrt_status gsrt_normal_noise(gsrt_ctx* ctx, uint64_t count, uint64_t seed, uint32_t stream_id, float* out);
/* the same, enqueued on gsrt_stream(); a device pointer only */
gsrt_status gsrt_normal_noise_async(gsrt_ctx* ctx, uint64_t count, uint64_t seed, uint32_t stream_id, float* d_out);
/* The optimiser state across a gsrt_densify: row i, i < n_out, of every present array of `out` is row origin[i] of `in`,
 * bit for bit, where origin[i] >= 0, and +0 in every word where origin[i] < 0 (a newly made Gaussian starts with fresh
 * moments): one gather over a whole gsrt_model_arrays (the layout the moments m and v of gsrt_model_step have). origin is
 * gsrt_densify's; an entry >= 0 must be a row of `in`, whose length the call is not told. Pointer and presence rules and
 * refusals as for gsrt_model_deactivate with `in` the input and `out` the output, except that no array of `out` may
 * overlap one of `in` (the gather is not in place); origin lives on the side, host or device, of the arrays. */
gsrt_status gsrt_model_remap(gsrt_ctx* ctx, uint32_t n_out, const int32_t* origin, const gsrt_model_arrays* in,
                             const gsrt_model_arrays* out);
gsrt_status gsrt_model_remap_async(gsrt_ctx* ctx, uint32_t n_out, const int32_t* d_origin, const gsrt_model_arrays* in,
                                   const gsrt_model_arrays* out);

/* ---- photometric loss: L1 + D-SSIM of a frame against a target image, with its gradient ---------
 * The loss of 3DGS's training step in one fused call: rgba is a frame as the renderer leaves it (float[H][W][4], used as
 * it is, no clamp; alpha is not read), target a float[H][W][target_channels] image with 3 or 4 channels (a fourth is not
 * read). Over the N = 3 H W colour values x of rgba and y of target:
 *     l1   = mean |x - y|,   mse = mean (x - y)^2   (so that PSNR = -10 log10(mse) comes free)
 *     ssim = mean of map, 3DGS's SSIM per channel: with conv the 11 x 11 Gaussian window (sigma 1.5; the product of two
 *            entries of gsrt_image_loss_window's table) over the image padded with 5 zeros on every side (conv2d(padding=5):
 *            border pixels see zeros, the window is not renormalised),
 *                mu1 = conv(x), mu2 = conv(y), s1 = conv(x x) - mu1^2, s2 = conv(y y) - mu2^2, s12 = conv(x y) - mu1 mu2,
 *                map = ((2 mu1 mu2 + C1) (2 s12 + C2)) / ((mu1^2 + mu2^2 + C1) (s1 + s2 + C2)),  C1 = 0.01^2, C2 = 0.03^2
 *     loss = (1 - lambda) l1 + lambda (1 - ssim),   lambda in [0, 1] (3DGS: 0.2)
 * out = {loss, l1, ssim, mse}. The per-pixel terms are float32 (every operation rounded on its own except the window
 * sums, which are fused multiply-adds, rows first, then columns); they are summed in double in a fixed order and each
 * scalar is rounded to float once.
 * grad_image (nullable): float[H][W][4] = d loss / d rgba, in the layout and meaning of the grad_image of
 * gsrt_render_splat_grad, gsrt_render_sh_grad and gsrt_render_opacity_grad, which take it as it is: per colour value
 *     (1 - lambda) / N * sign(x - y)  -  lambda / N * d (sum of map) / d x
 * with sign(0) = 0 (torch's convention; a NaN difference stays a NaN), the second term the exact derivative of the
 * formula above (zero padding included), and +0 in the alpha slot. The scale is that of the mean: a caller who weights
 * the loss multiplies the gradient by the same weight. Every pixel is a gather over its own 11 x 11 neighbourhood and
 * nothing is added atomically: the same inputs give the same bits, scalars and gradient alike. Without grad_image the
 * scalars are the same bits and the gradient pass is skipped.
 * rgba, target and grad_image are all host pointers or all device pointers (on the device rgba, grad_image and a
 * 4-channel target 16-byte aligned, as hipMalloc and torch give them); out is a host pointer. The call runs on
 * gsrt_stream(), behind the frame that wrote rgba (gsrt_framebuffer's pointer is a valid rgba), and blocks until out and
 * grad_image are complete. Any width, height >= 1 works, images smaller than the window included.
 * GSRT_E_ARG, with nothing written: a NULL ctx, rgba, target or out; width or height 0 or above 32768 (the renderer's
 * limit); target_channels not 3 or 4; lambda outside [0, 1] or NaN; host and device pointers mixed; grad_image
 * overlapping rgba or target. */
gsrt_status gsrt_image_loss(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* rgba, const float* target,
                            uint32_t target_channels, float lambda, float out[4], float* grad_image);
/* the same, enqueued on gsrt_stream() without a host synchronisation: it queues behind the frame that wrote d_rgba and
 * ahead of the gradient frame that reads d_grad_image. Device pointers only, d_out (4 floats) included. (A call for a
 * larger frame than any before it on this ctx allocates its workspace first.) */
gsrt_status gsrt_image_loss_async(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* d_rgba,
                                  const float* d_target, uint32_t target_channels, float lambda, float* d_out,
                                  float* d_grad_image);
/* the 1-D window of gsrt_image_loss: exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0..10, normalised to sum 1 in double and each
 * rounded to float once (a constant table; no device or ctx needed) */
gsrt_status gsrt_image_loss_window(float out[11]);

/* ---- frame loss: the photometric loss over a background, under a pixel mask, with a depth term ----
 * gsrt_image_loss with the three things a training frame needs beside it, each optional, in the same fused call. Per
 * pixel p of a width x height frame:
 *     a = rgba[p][3], read only with GSRT_LOSS_BACKGROUND or when depth is given (otherwise alpha is not read, junk and
 *         NaN included);   m = mask ? mask[p] : 1   (mask: float[H][W], any weights; 3DGS's alpha_mask)
 *     x_c  = rgb_c + (1 - a) * bg_c with GSRT_LOSS_BACKGROUND (bg = params.background), rgb_c without
 *     x'_c = m * x_c,  y'_c = m * y_c   with a mask; without one nothing is multiplied
 *     l1, mse, ssim: gsrt_image_loss's formulas on x', y' (the same window, the same zero padding, means over N = 3 H W)
 *     depth sample: depth given, target_depth[p] finite and > 0, and a >= alpha_min (a NaN alpha is no sample);
 *         on a sample, with D = depth[p] (the frame's premultiplied depth, gsrt_render_depth / gsrt_depth_buffer):
 *         q = D / a,  e = q - target_depth[p]
 *     depth_l1 = sum over samples of m |e| / (H W)   (3DGS's mean over all pixels),  depth_samples = their count
 *     loss = (1 - lambda) l1 + lambda (1 - ssim) + depth_weight * depth_l1
 * out = {loss, l1, ssim, mse, depth_l1, depth_samples}: per-pixel terms in float32, summed in double in a fixed order,
 * each scalar rounded to float once, as gsrt_image_loss does.
 * Gradients, in the layouts gsrt_render_splat_grad and gsrt_render_splat_depth_grad take as they are. g_c is
 * gsrt_image_loss's per-value gradient evaluated on x', y'; kd = (float)(depth_weight / (H W)) (the quotient in double):
 *     grad_image[p][c] = m * g_c
 *     grad_image[p][3] = B - (s * q) / a, where
 *         B = -(m * ((g_0 * bg_0 + g_1 * bg_1) + g_2 * bg_2)) with GSRT_LOSS_BACKGROUND and +0 without,
 *         s = (kd * m) * sign(e) on a depth sample, sign(0) = 0, and the second term is absent on any other pixel;
 *     grad_depth[p]    = s / a on a depth sample, +0 elsewhere
 * in float32, every operation rounded on its own in the order written (x_c = rgb_c + ((1 - a) * bg_c)); without a mask
 * every "m *" is left out, so that a mask of ones and no mask give the same bits. With neither background nor depth the
 * alpha slot is +0 and, with no mask either, the four shared scalars and grad_image are gsrt_image_loss's, bit for bit.
 * This is d(D / a): Gdepth / a into grad_depth and -Gdepth D / a^2 into the alpha slot, the division the depth frame
 * leaves to its caller. A gather without atomics: the same inputs give the same bits, scalars and both gradients.
 * grad_image (nullable) float[H][W][4]; grad_depth (nullable) float[H][W], needs depth and grad_image. All arrays are
 * host pointers or all device pointers (on the device rgba, grad_image and a 4-channel target 16-byte aligned); out is a
 * host pointer; the call runs on gsrt_stream() and blocks until the outputs are complete.
 * GSRT_E_ARG, with nothing written, named in gsrt_last_error: everything gsrt_image_loss refuses; a NULL params; an
 * unknown flag or a non-zero reserved; a NaN or infinite background with the flag set; depth_weight negative or NaN;
 * alpha_min outside (0, 1] or NaN; exactly one of depth and target_depth; grad_depth without depth or without
 * grad_image; host and device pointers mixed; an output overlapping an input or another output; a misaligned device
 * rgba, grad_image or 4-channel target.
 * Not provided: inverse-depth or scale-and-shift-invariant depth losses, other windows, multi-scale SSIM, a per-channel
 * mask. */
#define GSRT_LOSS_BACKGROUND 1u
#define GSRT_FRAME_LOSS_SCALARS 6
typedef struct gsrt_frame_loss_params {
    float lambda;          /* D-SSIM weight, [0, 1] */
    float background[3];   /* read with GSRT_LOSS_BACKGROUND */
    float depth_weight;    /* >= 0; weight of the depth term */
    float alpha_min;       /* (0, 1]; a pixel is a depth sample only when alpha >= this */
    uint32_t flags;
    uint32_t reserved;     /* zero */
} gsrt_frame_loss_params;
gsrt_status gsrt_frame_loss(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* rgba, const float* target,
                            uint32_t target_channels, const float* mask, const float* depth, const float* target_depth,
                            const gsrt_frame_loss_params* params, float out[GSRT_FRAME_LOSS_SCALARS], float* grad_image,
                            float* grad_depth);
/* the same, enqueued on gsrt_stream() without a host synchronisation, behind the frame that wrote d_rgba and d_depth and
 * ahead of the gradient frame that reads the two gradients. Device pointers only, d_out (6 floats) included. (A call for
 * a larger frame than any before it on this ctx allocates its workspace first.) */
gsrt_status gsrt_frame_loss_async(gsrt_ctx* ctx, uint32_t width, uint32_t height, const float* d_rgba,
                                  const float* d_target, uint32_t target_channels, const float* d_mask,
                                  const float* d_depth, const float* d_target_depth,
                                  const gsrt_frame_loss_params* params, float* d_out, float* d_grad_image,
                                  float* d_grad_depth);

/* ---- the optimiser step on the device: fused Adam over the raw model ------------------------------
 * With these calls this header alone describes a 3DGS training loop: gsrt_render, gsrt_image_loss, gsrt_render_splat_grad,
 * gsrt_splat_grad_to_model, gsrt_render_sh_grad, gsrt_model_step, gsrt_scene_update + gsrt_refit_bvh + gsrt_scene_set_sh
 * (INTEGRATION.md gives it in C). What is optimised, and what a .ply holds, is the raw model: a gsrt_model_arrays whose
 * rot_rxyz is an unnormalised quaternion, whose scale is the log scale and whose opacity is the logit; centre, sh and
 * features are stored as they are. The library's own model (gsrt_scene_from_model, gsrt_densify, gsrt_ply_read) is the
 * activated one. Everything is float32, every operation rounded on its own (no fused multiply-add), divisions and square
 * roots correctly rounded; no atomics: a result is a pure function of its inputs.
 * Activation, per Gaussian, of raw (r, x, y, z), log scale l_k and logit t:
 *     nq = sqrtf(((r r + x x) + y y) + z z),  q = raw_rot / nq (nq == 0 leaves q = raw_rot: the scene build's polynomial
 *     turns the zero quaternion into R = I),  s_k = expf(l_k),  o = 1 / (1 + expf(-t));
 * params_out[g] and aabbs_out[g] are, bit for bit, what gsrt_scene_from_model writes for (centre, q, s, o).
 * Chain, with dcov = grads.cov[g] (cov3d's order; an off-diagonal slot is one variable), R the scene build's rotation
 * matrix of q (Sigma_ij = sum_k s_k^2 R_ki R_kj) and D the symmetric matrix of dcov (an off-diagonal entry half its slot):
 *     w_k = D R_k,  d s_k = (2 s_k) (R_k . w_k),  d log_scale_k = d s_k * s_k,
 *     d R_ka = ((2 s_k) s_k) w_ka,  d q_c = sum_ka d R_ka dR_ka/dq_c,  d raw_rot = (dq - q (q . dq)) / nq, +0 when nq == 0,
 *     d logit = (grads.splat[g][5] * o) * (1 - o),
 *     d centre = grads.center[g], d sh and d features the table entries, unchanged.
 * Adam, per parameter word p with gradient g and its group's rate lr, with gsrt_adam_scalars' a1 = 1 - beta1,
 * a2 = 1 - beta2, c2 = sqrt(1 - beta2^t), ss = lr / (1 - beta1^t):
 *     m' = beta1 * m + a1 * g,   v' = beta2 * v + (a2 * g) * g,   p' = p - (ss * m') / (sqrtf(v') / c2 + eps).
 * The groups: centre, rot, log scale, logit, SH coefficient 0 of each channel (lr_sh_dc), SH coefficients 1..15
 * (lr_sh_rest), features. A group whose lr is exactly 0 is frozen: its raw, m and v words keep their bits. With
 * GSRT_ADAM_SPARSE a Gaussian that was not seen keeps every raw, m and v word bit for bit (3DGS's sparse Adam); "seen" is
 * gsrt_density_stats_add's: any of its splat row's slots 0..5 != 0.0f. Without the flag every Gaussian is stepped.
 * Not provided: other optimisers, learning-rate schedules beside gsrt_lr_expon (change lr_* per call), weight decay. */
#define GSRT_ADAM_SPARSE 1u
typedef struct gsrt_adam_params {
    float lr_center, lr_rot, lr_scale, lr_opacity, lr_sh_dc, lr_sh_rest, lr_features;
    float beta1, beta2, eps;      /* 3DGS: 0.9, 0.999, 1e-15 */
    uint32_t step;                /* t >= 1 */
    uint32_t flags;               /* GSRT_ADAM_SPARSE */
    uint32_t reserved[4];         /* zero, otherwise GSRT_E_ARG */
} gsrt_adam_params;

typedef struct gsrt_model_grads {     /* with respect to the activated model, as the library's backward writes them */
    const float* center;    /* n x 3: gsrt_splat_grad_to_model's grad_center (or the depth form's) */
    const float* cov;       /* n x 6: its grad_cov */
    const float* splat;     /* n x 8: the gradient frame's rows; slot 5 is d/d opacity, slots 0..5 decide "seen" */
    const float* sh;        /* n x 48 [gauss][coef][rgb]: gsrt_render_sh_grad's table; NULL exactly when the model has no sh */
    const float* features;  /* n x C: gsrt_render_feature_grad's table; NULL exactly when it has no features */
} gsrt_model_grads;

/* The float32 scalars the step's kernels use, host only (no ctx, no device): out = {1 - beta1, 1 - beta2,
 * sqrt(1 - beta2^t), then lr / (1 - beta1^t) for lr_center, lr_rot, lr_scale, lr_opacity, lr_sh_dc, lr_sh_rest,
 * lr_features}, each formed in double and rounded to float once. GSRT_E_ARG: a NULL pointer; step == 0; beta1 or beta2
 * outside [0, 1) or NaN; eps not > 0; a negative or NaN learning rate; a non-zero reserved word; an unknown flag. */
#define GSRT_ADAM_SCALARS 10
gsrt_status gsrt_adam_scalars(const gsrt_adam_params* adam, float out[GSRT_ADAM_SCALARS]);
/* One optimiser step of n Gaussians. raw, m (first moments) and v (second moments; the same layout as raw) are updated in
 * place; grads is read as the library's backward leaves it. Each of the outputs is nullable: act (as a whole, and, when
 * given, it has every array raw has) receives the activated model in the gsrt_scene_from_model convention, params_out
 * (n entries) and aabbs_out (n entries) the scene arrays, all three for all n Gaussians, stepped or not, activated from
 * the updated raw values; grad_raw (n x 11 floats: centre 3, rot 4, log scale 3, logit 1) the chained gradient the step
 * used, for every Gaussian. act->sh may be raw->sh itself and act->features raw->features itself (they are stored as
 * they are: nothing is copied then); otherwise the updated rows are copied.
 * raw, m, v and act must agree on feature_channels and on which of sh and features are present, and grads->sh /
 * grads->features are NULL exactly when the model has none. All arrays are host pointers, or all are device pointers
 * (ordinary device memory; whole float4 / float2 accesses are used where the bases are 16- / 8-byte aligned, as hipMalloc
 * and torch give them, dword accesses otherwise); the host form stages them in a device block of the call's.
 * The call runs on gsrt_stream(), behind the gradient calls that filled grads; the blocking form returns when everything
 * is written. After the async form call gsrt_synchronize before handing params_out / aabbs_out to gsrt_scene_update or
 * gsrt_scene_attach: those read their source on other streams.
 * GSRT_E_ARG, with nothing written: a NULL ctx, raw, m, v, grads or adam, or a NULL required array with n > 0; host and
 * device pointers mixed; what gsrt_adam_scalars refuses; sh or features presence, or the channel count (above
 * GSRT_MAX_FEATURES included), disagreeing between the structs; n > GSRT_MAX_GAUSSIANS; an output array overlapping an
 * input or another output (raw, m and v, written in place, must not overlap each other or grads either). */
gsrt_status gsrt_model_step(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw, const gsrt_model_arrays* m,
                            const gsrt_model_arrays* v, const gsrt_model_grads* grads, const gsrt_adam_params* adam,
                            const gsrt_model_arrays* act, gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out,
                            float* grad_raw);
/* the same, enqueued on gsrt_stream() without a host synchronisation; device pointers only */
gsrt_status gsrt_model_step_async(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw, const gsrt_model_arrays* m,
                                  const gsrt_model_arrays* v, const gsrt_model_grads* grads, const gsrt_adam_params* adam,
                                  const gsrt_model_arrays* act, gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out,
                                  float* grad_raw);
/* gsrt_model_step with an active SH degree, 3DGS's ramp-up (it starts at 0 and raises the degree every 1000 iterations):
 * sh_degree in 0..3. The words >= 3 (sh_degree + 1)^2 of each Gaussian's SH row are frozen: those words of raw->sh, m->sh
 * and v->sh keep their bits, exactly as a group with rate 0 does. The words below are stepped with gsrt_model_step's
 * arithmetic (lr_sh_dc for coefficient 0, lr_sh_rest for the others; the bias corrections use adam->step either way), and
 * everything else is gsrt_model_step's: act rows and the scene arrays are written for all words. sh_degree == 3 is
 * gsrt_model_step bit for bit (that call is this one with 3). A model without SH ignores the degree.
 * The frames still evaluate all 16 coefficients: a model whose inactive rows are zero (3DGS's initialisation, what
 * gsrt_train makes of SfM points) receives no gradient there from a frozen zero and renders as the lower degree does; a
 * model loaded with non-zero inactive rows keeps showing them, frozen.
 * GSRT_E_ARG also: sh_degree > 3. */
gsrt_status gsrt_model_step_degree(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw, const gsrt_model_arrays* m,
                                   const gsrt_model_arrays* v, const gsrt_model_grads* grads, const gsrt_adam_params* adam,
                                   uint32_t sh_degree, const gsrt_model_arrays* act, gsrt_gauss_param* params_out,
                                   gsrt_aabb* aabbs_out, float* grad_raw);
gsrt_status gsrt_model_step_degree_async(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw,
                                         const gsrt_model_arrays* m, const gsrt_model_arrays* v,
                                         const gsrt_model_grads* grads, const gsrt_adam_params* adam, uint32_t sh_degree,
                                         const gsrt_model_arrays* act, gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out,
                                         float* grad_raw);
/* The activation and packing alone, for step 0 and after a densify: the same arithmetic, the same kernel code path; raw is
 * only read. act, params_out and aabbs_out as for gsrt_model_step, with its pointer and aliasing rules and refusals. */
gsrt_status gsrt_model_activate(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw, const gsrt_model_arrays* act,
                                gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out);
gsrt_status gsrt_model_activate_async(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* raw, const gsrt_model_arrays* act,
                                      gsrt_gauss_param* params_out, gsrt_aabb* aabbs_out);
/* Activated to raw, which turns a gsrt_ply_read result or a gsrt_densify output into the raw form: centre and rot copied
 * bit for bit (a normalised quaternion is a raw one), log scale = logf(s), logit = logf(o / (1 - o)); sh and features
 * copied (raw->sh may be act->sh itself, raw->features act->features itself). An opacity of 1 gives +inf, of 0 -inf.
 * Pointers, presence and aliasing rules and refusals as for gsrt_model_activate, with act the input and raw the output. */
gsrt_status gsrt_model_deactivate(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* act, const gsrt_model_arrays* raw);
gsrt_status gsrt_model_deactivate_async(gsrt_ctx* ctx, uint32_t n, const gsrt_model_arrays* act,
                                        const gsrt_model_arrays* raw);
/* 3DGS's opacity reset on the raw model: logit' = min(logit, L), L = (float)log(max_opacity / (1 - max_opacity)) formed in
 * double (a NaN logit stays a NaN), and both moment arrays of the opacities are set to +0 for every Gaussian. The three
 * arrays (n floats each) are all host or all device pointers. On gsrt_stream(); the blocking form returns when they are
 * written. GSRT_E_ARG: a NULL ctx or pointer (with n > 0), mixed pointers, overlapping arrays, max_opacity outside (0, 1)
 * or NaN, n > GSRT_MAX_GAUSSIANS. */
gsrt_status gsrt_model_opacity_reset(gsrt_ctx* ctx, uint32_t n, float* logit_opacity, float* m_opacity, float* v_opacity,
                                     float max_opacity);
gsrt_status gsrt_model_opacity_reset_async(gsrt_ctx* ctx, uint32_t n, float* d_logit_opacity, float* d_m_opacity,
                                           float* d_v_opacity, float max_opacity);

/* 3DGS's get_expon_lr_func, host only (no ctx, no device): the log-linear decay from lr_init at step 0 to lr_final at
 * max_steps with the delayed start, computed in double and rounded to float once. With t = clamp(step / max_steps, 0, 1):
 *     lr = delay * exp(log(lr_init) (1 - t) + log(lr_final) t),
 *     delay = delay_steps > 0 ? delay_mult + (1 - delay_mult) sin(pi / 2 * clamp(step / delay_steps, 0, 1)) : 1,
 * and lr = 0 when lr_init and lr_final are both 0. GSRT_E_ARG: a NULL lr; max_steps == 0; a negative or NaN rate, or
 * exactly one of lr_init and lr_final zero; a NaN delay_mult. */
gsrt_status gsrt_lr_expon(float lr_init, float lr_final, float delay_mult, uint32_t delay_steps, uint32_t max_steps,
                          uint32_t step, float* lr);

/* ---- the training session: one object that owns a run's state on the device ------------------------
 * gsrt_trainer holds what a 3DGS training run carries from iteration to iteration, all of it in HBM: the raw model, both
 * Adam moment sets, the gradient tables, the densification statistics, the scene with its BVH, and the step counter. Its
 * calls are the sequences the entry points above compose to, with the stream ordering their comments ask for applied once,
 * here. Everything is allocated for `capacity` rows at creation (two sets of raw, m and v for the out-of-place densify,
 * the tables, noise, origin, stats, the scene arrays of a step); only the frame-sized buffers are regrown, when the frame
 * size changes. One trainer per ctx at a time is the tested use; calls on one trainer are serialised by the caller, like
 * every call on its ctx.
 * gsrt_trainer_create: model is the activated model (gsrt_scene_from_model's convention; host or device pointers, all on
 * one side), n of `capacity` rows used. The raw model is gsrt_model_deactivate of it, the moments, the statistics and
 * the screen radii (`capacity` floats) are +0, the active SH degree is 3, the scene is gsrt_scene_from_model of the model as given, with its BVH built. GSRT_E_ARG: a NULL pointer; a model with
 * features; n == 0; capacity < n; capacity > GSRT_MAX_GAUSSIANS.
 * gsrt_trainer_step: one iteration against one view. In order, all on gsrt_stream(): a COR frame of ubo with k
 * (gsrt_render_async; with target_depth a depth frame, gsrt_render_depth_async); gsrt_frame_loss_async of it against
 * target (width x height x target_channels), mask (nullable) and target_depth (nullable) with params: with no option set
 * its first four scalars and its gradient are gsrt_image_loss's; gsrt_render_splat_grad_async (with target_depth
 * gsrt_render_splat_depth_grad_async); gsrt_view_stats_add_async into the trainer's statistics (the bits
 * gsrt_density_stats_add_async leaves) and screen radii; the matching gsrt_splat*_grad_to_model_async; for a model with SH
 * gsrt_render_sh_grad_async; gsrt_model_step_degree_async with adam and the trainer's SH degree, whose
 * .step is ignored: the step number is the trainer's counter + 1. Then gsrt_synchronize, gsrt_scene_update with the
 * step's scene arrays, gsrt_refit_bvh(scene, NULL) and, with SH, gsrt_scene_set_sh, so that the next frame of the scene is
 * the stepped model's; the counter advances. scalars (host, nullable) receives gsrt_frame_loss's six. A step synchronises
 * with the host once in gsrt_synchronize (the scalars are read behind it) and once where gsrt_scene_set_sh drains the
 * queued frames. target, mask and target_depth are all host pointers or all device pointers; host ones are copied into
 * buffers of the trainer's. What gsrt_frame_loss, gsrt_adam_scalars or one of the frames would refuse is refused before
 * anything is enqueued, with the trainer, its counter included, as it was (GSRT_E_ARG; gsrt_last_error of the ctx says
 * why): NULL ubo, target, params or adam; a bad frame size or samples == 0; target_channels not 3 or 4; bad loss or Adam
 * parameters; mixed pointers; a misaligned 4-channel device target; a scene that was given a triangle mesh.
 * gsrt_trainer_densify: noise = gsrt_normal_noise(6 n, seed, stream_id = the step counter); gsrt_model_activate of the raw
 * model; gsrt_densify_async with params and the trainer's statistics into the second buffer set; n_out is read back (one
 * uint32) and written to *n_out (nullable). When it exceeds the capacity: GSRT_E_ARG with nothing changed (model, moments,
 * statistics, scene, n). Otherwise gsrt_model_deactivate of the new model, gsrt_model_remap of m and of v by the pass's
 * origin, the statistics and the screen radii set to +0 (as 3DGS resets max_radii2D), a new scene with a new BVH created from the new model, and the old scene destroyed:
 * A SCENE HANDLE OBTAINED FROM gsrt_trainer_scene BEFORE THIS CALL IS DEAD AFTER IT. A densify that prunes every
 * Gaussian (n_out == 0) is refused the same way.
 * gsrt_trainer_densify_screen: the same sequence with gsrt_densify_screen_async, the trainer's screen radii and
 * max_screen_radius (NaN: GSRT_E_ARG); gsrt_trainer_densify is this call with 0.
 * gsrt_trainer_set_sh_degree / gsrt_trainer_sh_degree: the active SH degree of the following steps (gsrt_model_step_degree;
 * 3 at creation). d > 3 is GSRT_E_ARG; without SH a degree is accepted and ignored.
 * gsrt_trainer_opacity_reset: gsrt_model_opacity_reset on the raw model and the moments, then the scene's arrays from
 * gsrt_model_activate, so that the next frame shows it.
 * gsrt_trainer_rebuild_bvh: gsrt_build_bvh of the scene, for callers whose Gaussians have moved far; a step only refits
 * (the topology is kept), and the trainer never rebuilds on its own.
 * gsrt_trainer_scene: the trainer's scene, borrowed, for evaluation views (gsrt_render, gsrt_pose_grad, ...); not to be
 * destroyed, updated or given a mesh or features by the caller. gsrt_trainer_info: n, capacity and the step counter (each
 * nullable). gsrt_trainer_state: the device addresses, borrowed and valid until the next gsrt_trainer_densify or
 * gsrt_trainer_destroy, of the raw model, the moments, the gradient tables of the last step and the statistics (n x 2);
 * each nullable. gsrt_trainer_radii: the screen radii (n floats in use), borrowed under the same rule.
 * gsrt_trainer_download: after draining the ctx, the raw model into raw_out and / or its activation
 * (gsrt_model_activate) into act_out: host arrays of n rows, sh NULL exactly when the model has none; either may be NULL.
 * Every call returns GSRT_E_ARG for a NULL trainer.
 * Not provided: features in a trainer; degree-limited frames (they evaluate all 16 SH coefficients); batched views; sharded frames; pose
 * refinement inside the trainer (gsrt_pose_grad remains callable on the borrowed scene); HIP graph capture of the step. */
typedef struct gsrt_trainer gsrt_trainer;
gsrt_status gsrt_trainer_create(gsrt_ctx* ctx, const gsrt_model_arrays* model, uint32_t n, uint32_t capacity,
                                gsrt_trainer** out);
void gsrt_trainer_destroy(gsrt_trainer* trainer);
gsrt_status gsrt_trainer_step(gsrt_trainer* trainer, const gsrt_ubo* ubo, uint32_t k, const float* target,
                              uint32_t target_channels, const float* mask, const float* target_depth,
                              const gsrt_frame_loss_params* params, const gsrt_adam_params* adam,
                              float scalars[GSRT_FRAME_LOSS_SCALARS]);
gsrt_status gsrt_trainer_densify(gsrt_trainer* trainer, const gsrt_densify_params* params, uint64_t seed, uint32_t* n_out);
gsrt_status gsrt_trainer_densify_screen(gsrt_trainer* trainer, const gsrt_densify_params* params, float max_screen_radius,
                                        uint64_t seed, uint32_t* n_out);
gsrt_status gsrt_trainer_set_sh_degree(gsrt_trainer* trainer, uint32_t sh_degree);
gsrt_status gsrt_trainer_sh_degree(const gsrt_trainer* trainer, uint32_t* sh_degree);
gsrt_status gsrt_trainer_radii(gsrt_trainer* trainer, const float** radii);
gsrt_status gsrt_trainer_opacity_reset(gsrt_trainer* trainer, float max_opacity);
gsrt_status gsrt_trainer_rebuild_bvh(gsrt_trainer* trainer);
gsrt_status gsrt_trainer_scene(gsrt_trainer* trainer, gsrt_scene** scene);
gsrt_status gsrt_trainer_info(const gsrt_trainer* trainer, uint32_t* n, uint32_t* capacity, uint32_t* step);
gsrt_status gsrt_trainer_state(gsrt_trainer* trainer, gsrt_model_arrays* raw, gsrt_model_arrays* m, gsrt_model_arrays* v,
                               gsrt_model_grads* grads, const float** stats);
gsrt_status gsrt_trainer_download(gsrt_trainer* trainer, const gsrt_model_arrays* raw_out, const gsrt_model_arrays* act_out);

/* ---- camera pose gradients: the backward of a frame to the model-view matrix -----------------------
 * The training loop above takes the cameras as known. For pose refinement and tracking (noisy COLMAP poses, SLAM,
 * relocalisation) gsrt_pose_grad chains the splat rows of gsrt_render_splat_grad (depth == 0) or of
 * gsrt_render_splat_depth_grad (depth != 0) to the camera: grad_model_view receives the partial derivative of the loss with
 * respect to each of the 16 floats of ubo.model_view, in the ubo's own column-major layout (entry c * 4 + r is row r,
 * column c), WITH ubo.model_view_inverse HELD FIXED. The renderer uses the two fields for separate things: model_view
 * feeds the projection (ppx, ppy, the conic, the depth key and the blended depth), model_view_inverse makes the rays
 * (origin and direction, hence the AABB slab test and the SH basis). The result is everything that flows through the splat
 * rows. Not differentiated, as for gsrt_render_splat_grad: the hits taken and their order, the AABB test, the cuts and the
 * stop. For a scene without SH rows, or with constant colour, it is the whole gradient of what is differentiated.
 * Per valid Gaussian g, gsrt_splat_grad_to_model's float32 quantities are recomputed in the same order: gt[0..3] = dL/dt at
 * the view-space position t = MV (c, 1), the (ppx, ppy) part through the general projection included (depth != 0:
 * gt[2] -= row[6]); g0[k] = dL/dT0[k], g1[k] = dL/dT1[k] at the Jacobian rows T0 = j02 MVz + j00 MVx, T1 = j12 MVz + j11 MVy.
 * Its contribution to grad_model_view[c * 4 + r], with c4 = (centre, 1):
 *     gt[r] * c4[c]                          for all r, c in 0..3 (the bottom row too: a float of the ubo like the others)
 *     + g0[c] * j00                          r = 0, c < 3          (T's own dependence on MV's 3x3)
 *     + g1[c] * j11                          r = 1, c < 3
 *     + (g0[c] * j02 + g1[c] * j12)          r = 2, c < 3
 * A Gaussian the projection marks invalid (depth <= 0 or det <= 0) contributes nothing. Each contribution is float32,
 * every operation rounded on its own. The 16 sums over the Gaussians are taken in double in an order that is a function
 * of n alone (fixed chunks of consecutive Gaussians, fixed trees; not of the grid, the device or timing), and each sum is
 * rounded to float once. No atomics: the same inputs give the same bits, as gsrt_image_loss promises for its scalars.
 * grad_splat (n x 8 floats) is a host or a device pointer; grad_model_view is a host pointer; the call blocks. The scene's
 * current parameters are read, as by gsrt_splat_grad_to_model. GSRT_E_ARG: a NULL pointer; a scene with a mesh.
 * GSRT_E_STATE: before gsrt_build_bvh. A refused call leaves grad_model_view as it was.
 * Not provided: gradients with respect to the projection matrix (intrinsics); the model_view_inverse partial, i.e. the ray
 * direction's effect on the SH basis (zero under a camera translation, since a pixel's world ray direction does not change;
 * under a rotation the term that pose-refining 3DGS systems drop as well); batched cameras (one call per view). */
gsrt_status gsrt_pose_grad(gsrt_scene* scene, const gsrt_ubo* ubo, const float* grad_splat, int depth,
                           float grad_model_view[16]);
/* the same, enqueued on gsrt_stream() behind the gradient frame; device pointers only (16 floats of ordinary device memory) */
gsrt_status gsrt_pose_grad_async(gsrt_scene* scene, const gsrt_ubo* ubo, const float* d_grad_splat, int depth,
                                 float* d_grad_model_view);
/* Host-only helpers for optimising a pose on the manifold (no ctx, no device; computed in double, each result rounded to
 * float once). gsrt_pose_twist: the gradient in the tangent space of a left (camera-frame) perturbation
 * MV' = exp(xi^) MV, xi = (v, w): with H = G MV^T as 4x4 matrices (G = grad_model_view),
 *     twist = { H[0][3], H[1][3], H[2][3],  H[2][1] - H[1][2], H[0][2] - H[2][0], H[1][0] - H[0][1] }    dL/dv, dL/dw.
 * gsrt_ubo_apply_twist: the retraction, model_view <- exp(xi^) model_view and model_view_inverse <- model_view_inverse
 * exp(-xi^), exp(xi^) = [[R, V v], [0, 1]] by Rodrigues' formula (by its series for |w| < 0.1). Nothing assumes that MV
 * is rigid. A zero twist leaves every bit of the ubo as it was. GSRT_E_ARG: a NULL pointer. */
gsrt_status gsrt_pose_twist(const float model_view[16], const float grad_model_view[16], float twist[6]);
gsrt_status gsrt_ubo_apply_twist(gsrt_ubo* ubo, const float twist[6]);

/* counters of the last render with GSRT_FLAG_STATS: [0] rays, [1] sum candidates |C_r|, [2] sum blended
 * |H_r|, [3] terminated rays, [4] tile collection rounds, [5] narrow-traversal restarts, [6] tiles,
 * [7] max candidates in one tile. Per-ray uint4 {candidates, blended, rounds, terminated} into
 * per_ray (host, W*H*4) when non-NULL. */
gsrt_status gsrt_last_stats(gsrt_ctx* ctx, uint64_t out[8], uint32_t* per_ray);
/* vulkan-sim's ray-tracing statistics (gpu-sim.cc:1510-1518) for the last REF render with GSRT_FLAG_STATS:
 * out = {rt_n_total_rays (traversals: rounds summed over the rays), rt_num_hits (traversals with a triangle hit),
 * rt_max_tree_depth, rt_max_nodes_per_ray, rt_tot_nodes_per_ray, walks that overflowed (0), 0, 0}. Nodes are
 * counted on gsrt's binary LBVH (internal nodes visited + leaves reached per traversal), so they compare in kind,
 * not in value, with the simulator's 6-wide Embree BVH. Per ray: gsrt_last_stats per_ray .y = triangle-hit
 * traversals, .w = nodes of one traversal. gsrt_dump_vs_stats writes the simulator's "rt_... = v" lines. */
gsrt_status gsrt_vs_stats(gsrt_ctx* ctx, uint64_t out[8]);
gsrt_status gsrt_dump_vs_stats(gsrt_ctx* ctx, const char* path);
/* the ExpLUT of REF mode (generateExpLUT(256, 0, 8), ExpLUT.hpp:10-24 / Scene.cpp:47): 256 x {k, b}.
 * as the host computes it (no device needed); gsrt_create uploads it for the kernels */
gsrt_status gsrt_exp_lut(float out[512]);

/* HIP-event timing of the next `frames` renders on gsrt_stream() (0 disables): per frame the render
 * kernel alone (REF: k_render_ref; COR: k_render_cor, after the first-round list kernel k_collect_cor)
 * and the whole frame (projection + list + render [+ gather/unpack]). gsrt_timing_read waits for
 * the stream and returns the recorded frames (at most `cap`). */
gsrt_status gsrt_timing(gsrt_ctx* ctx, uint32_t frames);
gsrt_status gsrt_timing_read(gsrt_ctx* ctx, float* kernel_ms, float* frame_ms, uint32_t cap, uint32_t* nframes);
/* per recorded frame, the exchange of a gsrt_render_sharded_async frame on gsrt_comm_stream(): from the moment the
 * rank's share is rendered to the end of the gather (+ rank 0's unpack), in ms; 0 for frames without an exchange.
 * Waits for the render and comm streams. */
gsrt_status gsrt_timing_read_exchange(gsrt_ctx* ctx, float* exchange_ms, uint32_t cap, uint32_t* nframes);
/* on != 0: the timed frames record only the render kernel's two events (frame_ms then reads 0), so that the timing
 * adds as little as possible to the frames it measures; 0 (default): all of them. Takes effect at gsrt_timing. */
gsrt_status gsrt_timing_kernel_only(gsrt_ctx* ctx, int on);
/* stride >= 1: of the frames after gsrt_timing, record the events of frames 0, stride, 2 stride, ... only (the
 * `frames` of gsrt_timing count recorded frames); 1 (default): every frame. Takes effect at gsrt_timing. */
gsrt_status gsrt_timing_stride(gsrt_ctx* ctx, uint32_t stride);

/* ---- multi-GPU tile sharding ------------------------------------------------ */
/* RCCL unique id (128 bytes) created on rank 0 and shipped to the other ranks by the caller */
gsrt_status gsrt_comm_unique_id(uint8_t out[128]);
gsrt_status gsrt_comm_init(gsrt_ctx* ctx, const uint8_t id[128], int nranks, int rank);
/* ranks of the ctx's communicator and this rank in it, from RCCL itself (ncclCommCount / ncclCommUserRank);
 * 1 / 0 without gsrt_comm_init. rank may be NULL. */
gsrt_status gsrt_comm_size(gsrt_ctx* ctx, int* nranks, int* rank);
/* the HIP stream (hipStream_t) on which a sharded frame's gather and rank 0's unpack into the framebuffer run,
 * or NULL when frames render straight into the framebuffer (one rank, or no gsrt_comm_init): work that reads a
 * gsrt_render_sharded_async frame's image goes on this stream (or after gsrt_synchronize) */
void* gsrt_comm_stream(gsrt_ctx* ctx);
/* render this rank's band of the frame (below), then ncclGather the tiles to rank 0, which unpacks them into its
 * framebuffer (and rgba_out, host or device, when non-NULL on rank 0). Every rank calls it for every frame.
 * With GSRT_FLAG_OUT_DUMP8 (COR) the tiles travel as dump codes instead (below): rank 0 reads the frame with
 * gsrt_dump8_read, and rgba_out must be NULL. */
gsrt_status gsrt_render_sharded(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k,
                                float* rgba_out);
gsrt_status gsrt_render_sharded_async(gsrt_scene* scene, const gsrt_ubo* ubo, uint32_t mode, uint32_t k);
/* The partition of a sharded frame: one band of whole tile rows per rank, rank r owning rows
 * [bands[r], bands[r + 1]) of every column (bands[0] = 0, bands[nranks] = tiles_y, non-decreasing). A rank's tiles are
 * numbered in the spatial order (super-tiles of 16x16 tiles, row-major) of its band's own grid; that is the order of
 * its block in the gather. On a communicator of N > 1 ranks the bands follow the shading cost: every 8th COR frame
 * the render kernel records each tile row's cost, one ncclAllReduce gives every rank the whole profile, and 8 frames
 * later every rank cuts the same new bands from it (gsrt_tile_bands' rule), kept only when they lower the heaviest
 * band's cost by 2 %. Profile frames follow a fixed schedule (every 8th sharded COR frame, pinned bands or not), and
 * the profile carries a hash of each rank's partition and pinning; ranks that disagree get GSRT_E_COMM.
 * A communicator holds at most 64 ranks (gsrt_comm_init returns GSRT_E_ARG beyond). */
/* tile decomposition of a frame under the even partition (no cost profile): out = {tile_w, tile_h, tiles_x, tiles_y,
 * tiles of `rank` among `nranks`, in-wave samples per pixel, first tile row of `rank`'s band, packed stride (the
 * largest band's tile count: the per-rank block size in the gathered buffer)}. Host-only. */
gsrt_status gsrt_tile_plan(const gsrt_ubo* ubo, uint32_t mode, int nranks, int rank, uint32_t out[8]);
/* the bands (nranks + 1 boundaries) the balancing rule cuts from a per-tile-row cost profile (tiles_y entries; NULL:
 * every row costs the same): each rank's summed row cost over its weight as even as whole rows allow, rank 0 (the
 * gather's root, which also receives and unpacks the frame) weighted 1 - 0.09 (nranks - 1) / spp (>= 1/4) in COR
 * mode (0.07 for GSRT_FLAG_OUT_DUMP8's 4-byte pixels); every band gets a row when tiles_y >= nranks. Host-only and deterministic. */
gsrt_status gsrt_tile_bands(const gsrt_ubo* ubo, uint32_t mode, int nranks, const uint32_t* row_cost, uint32_t* bands);
/* pin the partition of this ctx's sharded frames to `bands` (nranks + 1 entries; every rank of the job must pin the
 * same), or back to automatic balancing with NULL. Needs gsrt_comm_init. */
gsrt_status gsrt_set_bands(gsrt_ctx* ctx, int nranks, const uint32_t* bands);
/* the bands of the last sharded frame on this ctx (n = nranks + 1 entries, at most cap written; n = 0 before any) */
gsrt_status gsrt_last_bands(gsrt_ctx* ctx, uint32_t* bands, uint32_t cap, uint32_t* n);
/* the per-tile-row shading cost of the last whole (unsharded) COR frame: per tile, the candidates it staged plus a
 * constant, summed over the row (the profile the balancing uses). Waits for the frame. */
gsrt_status gsrt_row_costs(gsrt_ctx* ctx, uint32_t* row_cost, uint32_t cap, uint32_t* rows);

/* ---- the compact exchange format (GSRT_FLAG_OUT_DUMP8) -----------------------------------------
 * A sharded COR frame rendered with GSRT_FLAG_OUT_DUMP8 travels and stays as what its PPM dump prints: per pixel one
 * code word, 10 bits per channel holding rint(channel * 255) (bits 0-9 r, 10-19 g, 20-29 b), when every channel's
 * product is a finite, non-negative (not -0) number that rounds to at most 1022. Any other pixel has bit 30 set and
 * its exact r, g, b in an escape entry. gsrt_dump8_ppm of a frame's codes and escapes is byte-identical to
 * gsrt_dump_ppm of the same frame in RGBA32F. Each rank's block holds up to max(256, pixels / 64) escapes; a frame
 * with more fails at gsrt_dump8_read (GSRT_E_STATE) and is rendered again without the flag. */
typedef struct { uint32_t pixel; float r, g, b; } gsrt_dump8_escape;  /* pixel = x + y * width */
#define GSRT_DUMP8_ESCAPE (1u << 30)
/* rank 0, after a GSRT_FLAG_OUT_DUMP8 sharded frame: its width x height code words (codes may be NULL) and its escapes
 * in pixel order (at most cap written; n_esc = how many the frame has). Waits for the frame. */
gsrt_status gsrt_dump8_read(gsrt_ctx* ctx, uint32_t* codes, gsrt_dump8_escape* esc, uint32_t cap, uint32_t* n_esc);
/* host: the code words of an RGBA32F frame (n pixels), and the escapes it needs (at most cap written, n_esc all) */
gsrt_status gsrt_dump8_encode(const float* rgba, size_t n, uint32_t* codes, gsrt_dump8_escape* esc, uint32_t cap,
                              uint32_t* n_esc);
/* host: the P3 PPM of a frame in codes + escapes (the bytes gsrt_dump_ppm writes for the frame) */
gsrt_status gsrt_dump8_ppm(const char* path, const uint32_t* codes, uint32_t width, uint32_t height,
                           const gsrt_dump8_escape* esc, uint32_t n_esc);

/* ---- frame dump (replaces VulkanRayTracing::image_store, vulkan_ray_tracing.cc:2203-2247) ---- */
/* P3 PPM, "%3.0f %3.0f %3.0f\n" of rgb*255 per pixel, host rgba pointer */
gsrt_status gsrt_dump_ppm(const char* path, const float* rgba, uint32_t width, uint32_t height);
/* "<dd-mm-YYYY-HH-MM-SS->SCENE.ppm" name the reference derives from local time */
gsrt_status gsrt_reference_ppm_name(char* out, size_t cap);
/* dump_image.sh text: "[x, y] rgba(r, g, b)" per pixel, the RayTracing.rgen:98 debugPrintf line
 * (RTV/dump_image.sh keeps the lines containing "rgba"), rows top to bottom */
gsrt_status gsrt_dump_rgba_text(const char* path, const float* rgba, uint32_t width, uint32_t height);
/* Intel-path image.binary records {float r, g, b; uint32 offset = x + y*W} (vulkan_ray_tracing.cc:2165-2179) */
gsrt_status gsrt_dump_image_binary(const char* path, const float* rgba, uint32_t width, uint32_t height);
/* Portable float map of a host image with 1 ("Pf") or 3 ("PF") channels per pixel, e.g. a depth image: header
 * "Pf\nW H\n-1.0\n" (negative scale: little-endian float32), then the rows bottom to top */
gsrt_status gsrt_dump_pfm(const char* path, const float* data, uint32_t width, uint32_t height, uint32_t channels);



#ifdef __cplusplus
}
#endif
#endif /* GSRT_H */
