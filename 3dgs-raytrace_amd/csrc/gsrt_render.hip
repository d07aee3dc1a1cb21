// gsrt_render.hip -- the hot path: per-ray Gaussian intersection + alpha compositing.
//
// Reference path: GaussTracing.rgen round loop -> VulkanRayTracing::traceRay (DFS over
// the Embree BVH, exact slab test, every procedural AABB hit becomes a candidate) ->
// RayTracing.ProceduralGauss.rint per candidate (EWA, LinearExp, K=8 insert) -> .rchit (transmittance).
//
// MI355X design: one wavefront = one 64-ray packet of primary rays (a TW x TH pixel tile x S samples,
// TW*TH*S = 64), one tile per single-wave workgroup. Per tile:
//   1. packet traversal of the LBVH: the wave pops up to 64 nodes at a time from an LDS stack, each lane
//      tests its node's two child boxes against the tile frustum, hit children / leaves are compacted
//      with ballots (no per-lane stacks, no divergence);
//   2. leaf candidates become 64-bit keys in an LDS buffer; a wave bitonic sort orders them (COR: by
//      (depth, id) -- the front-to-back order the reference's K-nearest rounds produce; REF: by id);
//      when more than CAP candidates exist the buffer keeps the CAP nearest and the tile re-traverses
//      for the next CAP beyond the last key (the rgen round loop, done once per 64 rays);
//   3. the sorted candidates are shaded in groups staged through LDS: while group g is shaded (every lane
//      reads the same record: a broadcast), group g+1's records and SH coefficients are already in flight
//      as coalesced vector loads; every lane runs the exact VS slab test for its own ray and the EWA /
//      blend arithmetic.
// The BVH and the frustum are conservative filters; the per-lane slab test decides membership exactly
// as the reference does, so the result does not depend on the BVH, the tile shape or CAP.
//
// Kernel arguments (camera + argument block, ~100 dwords) are never kept live: every use site re-reads
// them with scalar loads through a laundered constant-address-space view of the kernarg segment (kargs()),
// which keeps the SGPR budget for the shading loop instead of spilling it into VGPR lanes.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <type_traits>

#include "gsrt_internal.hpp"
#include "gsrt_project.hpp"

namespace gsrt {

constexpr uint32_t kStack = 512;   // LDS node stack of the 64-wide traversal (entries)
// (kCap, kFG and kSG: gsrt_device.hpp, since the frame plan and the dispatch orders of gsrt_plan.cpp use them too)
constexpr uint32_t kGroup = 4;    // candidates per LDS stage
constexpr uint32_t kRCap = 128;    // k_render_cor's own traversal rounds (rare: past a group list's end)
constexpr uint32_t kRBuf = 2 * kRCap;
constexpr uint32_t kRStack = 256;
constexpr uint32_t kGCap = 896;    // candidates per group-list segment
#ifndef GSRT_GROUP_SEGMENTS
#define GSRT_GROUP_SEGMENTS 2
#endif
constexpr uint32_t kGSegs = GSRT_GROUP_SEGMENTS;  // segments of an overflowing group list (k_group_more)
constexpr uint32_t kGStride = kGSegs * kGCap;     // glist entries per group
constexpr uint32_t kMoreLanes = 16;               // k_group_more runs where a tile holds >= 16 samples per pixel
constexpr uint32_t kGBuf = 1024;   // group key buffer (a power of two >= kGCap + 128)
constexpr uint32_t kGStack = 432;  // LDS node stack of the group traversal: 432 entries keep the
                                           // kernel at 10 KB of LDS, 16 waves/CU (1080p: 8160 groups, 2 rounds)
constexpr uint32_t kNoGroup = 0xFFFFFFFFu;
// k_group_list sorts its final list in registers (wave_sort<true>); A/B builds set GSRT_GROUP_REGSORT=0 (LDS network)
#ifndef GSRT_GROUP_REGSORT
#define GSRT_GROUP_REGSORT 1
#endif
constexpr bool kGroupRegSort = GSRT_GROUP_REGSORT != 0;
// A/B knobs of the GRAD kernels (kGradWaves, shade_stage)
#ifndef GSRT_GRAD_WAVES
#define GSRT_GRAD_WAVES 5
#endif
#ifndef GSRT_GRAD_AB
#define GSRT_GRAD_AB 0
#endif
#ifndef GSRT_SHGRAD_WAVES
#define GSRT_SHGRAD_WAVES 4
#endif
#ifndef GSRT_OPGRAD_WAVES
#define GSRT_OPGRAD_WAVES 4
#endif
#ifndef GSRT_SPLATGRAD_WAVES
#define GSRT_SPLATGRAD_WAVES 3
#endif
#ifndef GSRT_SPLATDEPTHGRAD_WAVES
#define GSRT_SPLATDEPTHGRAD_WAVES 3
#endif
constexpr uint32_t kFront = 128;   // frontier entries per super-group


struct RenderArgs {
    const SplatRec* recs;
    const float* sh;                 // device layout [gauss][rgb][coef 16]
    const BvhNode* nodes;
    const float* lut;
    float* out;                      // framebuffer RGBA32F or packed tiles
    gsrt_raystate* rs;               // REF per-ray state (nullable)
    uint32_t* ray_stats;             // per-pixel uint4 (nullable)
    unsigned long long* counters;    // [0..7] stats, [8] error flags, [9..31] diagnostics (GSRT_DIAG)
    uint32_t n, root_ref;
    const float* root_box;           // device: 6 floats written by the fit (no host round trip per refit)
    uint32_t width, height, tiles_x, tiles_y, ntiles_local, rank, nranks;
    uint32_t row0, row1;             // this rank's band of tile rows (Bands): its local tiles (band_tile)
    uint32_t* tile_cost;             // COR: per local tile, its shading cost (the partition's profile), or nullptr
    // GSRT_FLAG_OUT_DUMP8 (packed COR frames): out holds one Dump8 code word per pixel, escapes go to esc (count at
    // esc[0].x, entries from esc[1]), passes > 1 sum into accum
    uint32_t dump8, esc_cap;
    uint4* esc;
    float4* accum;
    uint32_t tw, th, s_lanes, passes, packed, samples, bounces;
    uint32_t stack_limit;            // <= kStack; lowered only by the GSRT_DEBUG_STACK_LIMIT test knob
    uint32_t* lists;                 // COR: per local tile, the first round's sorted candidate ids (kCap)
    uint4* list_hdr;                 // per local tile: {count, total, last key lo, last key hi}
    uint32_t prelisted;              // 1: k_collect_cor filled lists/list_hdr for this frame
    uint32_t cull2d;                 // COR: drop listed candidates whose 2D footprint misses the tile (not with STATS)
    uint32_t leaf_fp;                // COR: leaf slots of the nodes hold footprint boxes (k_project): traversals test
                                     // those instead of the leaf AABB, and need no footprint cull afterwards
    uint32_t use_groups;             // COR: k_group_list builds the tile lists (else k_collect_cor per tile)
    uint32_t* frontier;              // per super-group: {count, kFront node ids} (k_frontier), or nullptr
    uint32_t sgroups_x, sgroups;
    uint64_t* glist;                 // per group: its sorted candidate keys (kGStride), for continuation rounds
    uint4* ghdr;                     // per group: {count | more << 31, 0, last key lo, hi}
    const float4* footprint;         // COR: per splat a kFpWords record: pixel box {x0, x1, y0, y1}, ellipse terms
                                     // e0, e1 (k_project)
    uint32_t groups_x, groups;       // tile groups of fg x fg tiles over the whole frame
    uint32_t fg;                     // tiles per group side (RenderPlan::fg: 4, or 2 with 4+ ranks)
    const uint32_t* group_order;     // k_group_list: workgroup -> group (centre first), or nullptr (row-major)
    RankTiles own;                   // sharded frames: the rank's tiles (k_frontier skips super-groups it does not own)
    const uint32_t* run_order;       // k_render_cor: dispatch order of the runs of kRun local tiles (xcd_local_tile_perm)
    const float* tri_t;              // REF with a mesh: closest triangle hit t per pixel (k_mesh_thit), or nullptr
    const uint32_t* depth_unsafe;    // COR: the scene's word k_project sets when a keyed centre lies outside its AABB's
                                     // depth bound (depth_lo): the traversals' depth cull is off while it is non-zero
    uint32_t depth_cull;             // the traversals' depth cull is on (where group lists overflow, launch_render)
    float* depth_out;                // COR with GSRT_FLAG_DEPTH: width x height floats, row-major (k_render_cor DEPTH);
                                     // after the members before it, so that no other member's kernarg offset moved
    // COR with GSRT_FLAG_FEATURES (k_render_cor FEAT), likewise appended: the image, width x height x feat_channels floats
    // (row-major, pixel-interleaved), and the scene's table, one 64-B row of 16 floats per Gaussian id
    float* feat_out;
    const float* feat_rows;
    uint32_t feat_channels;
    // COR gradient frames (GSRT_FLAG_FEATURE_GRAD, k_render_cor GRAD), likewise appended: the upstream gradient image,
    // width x height x grad_channels floats laid out as a feature image, and the gradient table the frame adds to, one
    // 64-B row of 16 floats per Gaussian id (zeroed before the frame, compacted after it: launch_grad_compact)
    // An SH gradient frame (GSRT_FLAG_SH_GRAD, k_render_cor shgrad) uses the same three: grad_in is the upstream gradient of
    // the RGBA frame (grad_channels = 4, the image's stride; alpha's is not read), grad_rows one 192-B row of 48 floats
    // per Gaussian id, [rgb][coef] as the SH rows are (compacted by launch_sh_grad_compact)
    // An opacity gradient frame (GSRT_FLAG_OPACITY_GRAD, k_render_cor opgrad) likewise: grad_in is the upstream gradient of
    // the RGBA frame, all four channels read, and grad_rows the caller's own table, one float per Gaussian id
    // A splat gradient frame (GSRT_FLAG_SPLAT_GRAD, k_render_cor splatgrad) likewise: grad_in as for opacity, grad_rows the
    // caller's own table, one 32-B row of 8 floats per Gaussian id
    const float* grad_in;
    float* grad_rows;
    uint32_t grad_channels;
    // A splat-depth gradient frame (GSRT_FLAG_SPLAT_DEPTH_GRAD, k_render_cor splatdepthgrad), likewise appended: grad_in and
    // grad_rows as for a splat gradient frame, and the upstream gradient of the depth image, width x height floats
    const float* grad_depth_in;
};

#ifdef GSRT_WAVE_TIMES
// diagnostic build (profiles/wave_times.py): per workgroup of the last launch {start, end} of the 100-MHz
// real-time counter, HW_ID and XCC_ID; [0] k_render_cor, [1] k_group_list
__device__ uint4 g_wave_times[2][1u << 18];
__device__ uint32_t g_stamps[4];  // real-time counter when the render stream reaches the render kernel / after it
__global__ void k_stamp(uint32_t i) { g_stamps[i] = (uint32_t)__builtin_amdgcn_s_memrealtime(); }
__device__ GSRT_INLINE void wave_time(uint32_t kind, uint32_t idx, uint32_t t0) {
    if (__lane_id() == 0 && idx < (1u << 18))
        g_wave_times[kind][idx] = make_uint4(t0, (uint32_t)__builtin_amdgcn_s_memrealtime(),
                                                    __builtin_amdgcn_s_getreg((31 << 11) | 4),
                                                    __builtin_amdgcn_s_getreg((31 << 11) | 20));
}
#define GSRT_WT_START const uint32_t wt_start = (uint32_t)__builtin_amdgcn_s_memrealtime()
#define GSRT_WT_END(kind, idx) wave_time(kind, idx, wt_start)
#else
#define GSRT_WT_START
#define GSRT_WT_END(kind, idx)
#endif

struct KArgs {                       // the single by-value kernel argument
    gsrt_ubo ubo;
    RenderArgs a;
};

// Fresh view of the kernel arguments: the asm makes the pointer opaque, so loads through it cannot be
// hoisted to kernel entry and stay short-lived scalar loads at each use site.
__device__ GSRT_INLINE const KArgs& kargs() {
    const __attribute__((address_space(4))) KArgs* p =
        (const __attribute__((address_space(4))) KArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const KArgs*)p;
}

// ---- tile order: spatial_tile / spatial_index / owner_of, kXcds and kDeal live in gsrt_device.hpp (the projection and
// the host's dispatch orders use them too)

// Workgroup b of a launch over nl local tiles -> local tile index. Under round-robin dispatch the
// workgroups of XCD x are b = x, x+8, ...; they are given whole runs of kRun consecutive tiles of the
// spatial order (one super-tile), runs dealt round-robin over the XCDs: an XCD's in-flight tiles share
// their Gaussians in its L2, and neighbouring runs (similar cost) run on all XCDs at once. A bijection on
// every complete round of 8 runs; the final partial round maps to itself.
__host__ __device__ GSRT_INLINE uint32_t xcd_local_tile(uint32_t b, uint32_t nl) {
    const uint32_t round_len = kXcds * kRun;
    if (b >= (nl / round_len) * round_len) return b;
    const uint32_t x = b % kXcds, i = b / kXcds;
    return ((i / kRun) * kXcds + x) * kRun + i % kRun;
}
// As xcd_local_tile, with units of kDeal consecutive tiles (a quarter super-tile) of the complete rounds taken in
// the order perm lists (centre-out: the costly units first, so the launch ends on short tiles); perm == nullptr:
// spatial order. A rank of a sharded frame has few runs (63 at 8 ranks, C3): dealt whole, the XCDs' shares
// differed by 25 % in cost; quarter runs balance them better and stay spatially coherent.
__device__ GSRT_INLINE uint32_t xcd_local_tile_perm(uint32_t b, uint32_t nl, const uint32_t* perm) {
    const uint32_t round_len = kXcds * kDeal;
    if (!perm || b >= (nl / round_len) * round_len) return xcd_local_tile(b, nl);
    const uint32_t x = b % kXcds, i = b / kXcds;
    return perm[(i / kDeal) * kXcds + x] * kDeal + i % kDeal;
}


// ---- frustum -------------------------------------------------------------------------------------

struct Frustum { float n[4][3]; float o[3]; };

__device__ GSRT_INLINE void cross3(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// Cone from the pinhole through the pixel rectangle [x0,x1] x [y0,y1] (already widened by a margin).
__device__ GSRT_INLINE Frustum make_frustum(const gsrt_ubo& u, float x0, float y0, float x1, float y1) {
    Frustum f;
    float d[4][3];
    gen_ray(u, x0, y0, f.o, d[0]);
    gen_ray(u, x1, y0, f.o, d[1]);
    gen_ray(u, x1, y1, f.o, d[2]);
    gen_ray(u, x0, y1, f.o, d[3]);
    const float c[3] = {d[0][0] + d[1][0] + d[2][0] + d[3][0], d[0][1] + d[1][1] + d[2][1] + d[3][1],
                        d[0][2] + d[1][2] + d[2][2] + d[3][2]};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        cross3(d[i], d[(i + 1) & 3], f.n[i]);
        const float s = f.n[i][0] * c[0] + f.n[i][1] * c[1] + f.n[i][2] * c[2];
        if (s < 0.0f) { f.n[i][0] = -f.n[i][0]; f.n[i][1] = -f.n[i][1]; f.n[i][2] = -f.n[i][2]; }
    }
    return f;
}

// true when the box lies strictly outside one side plane (positive-vertex test)
__device__ GSRT_INLINE bool box_outside(const Frustum& f, const float lo[3], const float hi[3]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = (f.n[p][k] >= 0.0f ? hi[k] : lo[k]) - f.o[k];
            s = fmaf(f.n[p][k], v, s);
        }
        if (s < 0.0f) return true;
    }
    return false;
}

// ---- wave helpers -------------------------------------------------------------------------------

__device__ GSRT_INLINE uint32_t popc_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ GSRT_INLINE uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// the lane id recomputed at this point (laundered): values derived from it in a rarely taken block are not
// hoisted out of the loops around it into long (spilled) live ranges
__device__ GSRT_INLINE uint32_t lane_here() {
    uint32_t l = lane_id();
    asm volatile("" : "+v"(l));
    return l;
}
__device__ GSRT_INLINE uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ GSRT_INLINE unsigned long long wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Wave-wide bitonic sort of keys[0..count) ascending in LDS (padded to a power of two with ~0).
// Bitonic sort of n = 64 R keys held in registers, element r * 64 + lane in v[r]: stages whose partner is in
// another lane exchange through __shfl_xor (no LDS round trip, no barrier), the others within a lane.
template <uint32_t R>
__device__ GSRT_INLINE void wave_sort_regs(uint64_t (&v)[R], uint32_t lane) {
    constexpr uint32_t n = 64 * R;
#pragma unroll
    for (uint32_t k = 2; k <= n; k <<= 1) {
#pragma unroll
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            if (j >= 64) {  // partner: register r ^ (j / 64) of the same lane
#pragma unroll
                for (uint32_t r = 0; r < R; ++r) {
                    const uint32_t q = r ^ (j / 64);
                    if (q <= r) continue;
                    const bool asc = k == n || ((r * 64) & k) == 0;  // (e & k) == 0 for e = r * 64 + lane
                    const uint64_t a = v[r], c = v[q];
                    const bool sw = (a > c) == asc;
                    v[r] = sw ? c : a;
                    v[q] = sw ? a : c;
                }
            } else {  // partner: lane ^ j, same register
                // the lane id laundered per stage: the stage's lane masks are formed here, not hoisted to the top of
                // the kernel as dozens of live SGPR pairs (spilled once the sort is inlined into its caller)
                uint32_t ln = lane;
                asm volatile("" : "+v"(ln));
                const bool lower = (ln & j) == 0;
#pragma unroll
                for (uint32_t r = 0; r < R; ++r) {
                    const uint32_t e = r * 64 + ln;
                    const bool asc = (e & k) == 0;
                    const uint64_t a = v[r];
                    const uint32_t plo = (uint32_t)__shfl_xor((int)(uint32_t)a, (int)j);
                    const uint32_t phi = (uint32_t)__shfl_xor((int)(uint32_t)(a >> 32), (int)j);
                    const uint64_t p = ((uint64_t)phi << 32) | plo;
                    const bool keep_min = lower == asc;
                    const bool a_small = a < p;
                    v[r] = (a_small == keep_min) ? a : p;
                }
            }
        }
    }
}

template <uint32_t R>
__device__ GSRT_INLINE void wave_sort_r(uint64_t* keys, uint32_t count, uint32_t lane) {
    uint64_t v[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t e = r * 64 + lane;
        v[r] = e < count ? keys[e] : ~0ull;
    }
    wave_sort_regs<R>(v, lane);
    __syncthreads();  // every lane has read its elements
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) keys[r * 64 + lane] = v[r];
    __syncthreads();
}

// Sort keys[0..count) ascending; keys[count..n) (n = count rounded up to a power of two) become ~0.
// REGS (k_group_list, where the sort is on the latency chain of every group): counts up to 1024 sort in
// registers (wave_sort_r, up to 32 VGPRs of keys; the kernel takes 104 VGPRs instead of 75, which costs no
// occupancy: its 10 KB of LDS hold it to 4 waves/SIMD, and beside the render kernel a group-list wave takes the
// slot of one retiring 80-VGPR render wave either way; C3 -0.8 %, C2 -0.6 % against sorting 513-1024 keys in
// LDS); otherwise (the render kernels' rare traversals, whose occupancy depends on their VGPR count) the LDS
// bitonic network below.
template <bool REGS = false>
__device__ GSRT_INLINE void wave_sort(uint64_t* keys, uint32_t count) {
    const uint32_t lane = lane_id();
    if constexpr (REGS) {
        count = __builtin_amdgcn_readfirstlane(count);
        if (count <= 64) { wave_sort_r<1>(keys, count, lane); return; }
        if (count <= 128) { wave_sort_r<2>(keys, count, lane); return; }
        if (count <= 256) { wave_sort_r<4>(keys, count, lane); return; }
        if (count <= 512) { wave_sort_r<8>(keys, count, lane); return; }
        if (count <= 1024) { wave_sort_r<16>(keys, count, lane); return; }
    }
    uint32_t n = 2;
    while (n < count) n <<= 1;
    for (uint32_t i = count + lane; i < n; i += 64) keys[i] = ~0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= n; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = lane; t < (n >> 1); t += 64) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const uint32_t l = i + j;
                const bool up = (i & k) == 0;
                const uint64_t a = keys[i], b = keys[l];
                if ((a > b) == up) { keys[i] = b; keys[l] = a; }
            }
            __syncthreads();
        }
    }
}

// keys[0..P) sorted ascending, keys[P..count) not (count <= BUF, BUF a power of two, BUF - P = 64 R): afterwards keys[0..BUF)
// is sorted ascending (keys[count..BUF) hold ~0 first). The tail is sorted in registers (R keys per lane) and written back
// descending, so that keys[0..BUF) is one bitonic sequence, which a single bitonic merge (log2 BUF half-cleaner stages
// over LDS) sorts: the overflow of a traversal's key buffer re-sorts its 128 new keys instead of all BUF.
template <uint32_t BUF, uint32_t P>
__device__ GSRT_INLINE void merge_tail(uint64_t* keys, uint32_t count) {
    static_assert((BUF & (BUF - 1)) == 0 && BUF > P && (BUF - P) % 64 == 0, "merge_tail: BUF - P a multiple of 64");
    constexpr uint32_t R = (BUF - P) / 64;
    const uint32_t lane = lane_id();
    uint64_t v[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t e = P + r * 64 + lane;
        v[r] = e < count ? keys[e] : ~0ull;
    }
    wave_sort_regs<R>(v, lane);
    __syncthreads();  // every lane has read its tail keys
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) keys[BUF - 1 - (r * 64 + lane)] = v[r];
    __syncthreads();
#pragma unroll 1
    for (uint32_t j = BUF >> 1; j > 0; j >>= 1) {
#pragma unroll 2
        for (uint32_t t = lane; t < (BUF >> 1); t += 64) {
            const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
            const uint64_t a = keys[i], b = keys[i + j];
            if (a > b) { keys[i] = b; keys[i + j] = a; }
        }
        __syncthreads();
    }
}

// ---- packet traversal ---------------------------------------------------------------------------

struct KeyRef {  // REF: candidates ordered by Gaussian id (the oracle's order)
    static constexpr bool kUsesDepth = false;
    __device__ GSRT_INLINE bool operator()(uint32_t, uint32_t gid, uint64_t& key) const { key = gid; return true; }
};
struct KeyCor {  // COR: (depth, id); invalid splats (behind the camera, singular: depth = +inf) never enter
    static constexpr bool kUsesDepth = true;
    __device__ GSRT_INLINE bool operator()(uint32_t depth_bits, uint32_t gid, uint64_t& key) const {
        key = ((uint64_t)depth_bits << 32) | gid;
        return depth_bits < 0x7f800000u;
    }
};
// COR inside k_render_cor: the same key, its depth read from the frame's own records. The leaf keys in the
// BVH nodes belong to the prep stage, which may already be writing the next frame's (FrameSlot).
struct KeyCorRec {
    static constexpr bool kUsesDepth = true;
    __device__ GSRT_INLINE bool operator()(uint32_t, uint32_t gid, uint64_t& key) const {
        return KeyCor{}(__float_as_uint(kargs().a.recs[gid].depth), gid, key);
    }
};

// pixel rectangle the tile's rays pass through (with margin)
struct TileRect { float x0, y0, x1, y1; };

__device__ GSRT_INLINE TileRect tile_rect(uint32_t tx, uint32_t ty, uint32_t tw, uint32_t th) {
    const uint32_t x0 = tx * tw, y0 = ty * th;
    return TileRect{(float)x0 - 0.5f, (float)y0 - 0.5f, (float)(x0 + tw) + 0.5f, (float)(y0 + th) + 0.5f};
}
// Footprint test of splat gid against a sample rectangle: its pixel box meets rect and the g-ellipse
// {g <= gcut} meets rect (k_project stores the ellipse widened by 2 % + 2e-3 in g). The rect is a TileRect (with
// its 0.5-px frustum margin); the samples lie in [x0 + 0.5, x1 - 0.5) and the footprints carry their own
// rounding margins, so the test uses the rect without the frustum margin.
constexpr float kFpInset = 0.5f;
// Exact ellipse-rectangle test. With d = p - centre and the ellipse q(d) = (A dx^2 + 2B dx dy + C dy^2) / T <= 1,
// q restricted to an edge dx = X is Cs (dy + kc X)^2 + Dc X^2 (Cs = C/T, kc = B/C, Dc = det/(C T)): a sum of two
// non-negative terms, no cancellation, minimised at dy = -kc X clamped to the edge; likewise for dy = Y edges.
// A convex q meets the rectangle iff its centre lies inside or its minimum over one of the four edges is <= 1.
// e0 = (cx, cy, kc, ka), e1 = (Cs, As, Dc, Da); the rectangle (x0, x1, y0, y1) is widened by kEllMargin.
constexpr float kEllMargin = 0.01f;
__device__ GSRT_INLINE float ell_edge(float X, float k, float s, float d, float lo, float hi) {
    const float m = -k * X;
    const float r = __builtin_amdgcn_fmed3f(m, lo, hi) - m;
    return fmaf(s * r, r, (d * X) * X);
}
__device__ GSRT_INLINE bool ell_meets(const float4 e0, const float4 e1, float x0, float x1, float y0, float y1) {
    const float ax = x0 - e0.x - kEllMargin, bx = x1 - e0.x + kEllMargin;
    const float ay = y0 - e0.y - kEllMargin, by = y1 - e0.y + kEllMargin;
    if (ax <= 0.0f && bx >= 0.0f && ay <= 0.0f && by >= 0.0f) return true;
    const float q = fminf(fminf(ell_edge(ax, e0.z, e1.x, e1.z, ay, by), ell_edge(bx, e0.z, e1.x, e1.z, ay, by)),
                          fminf(ell_edge(ay, e0.w, e1.y, e1.w, ax, bx), ell_edge(by, e0.w, e1.y, e1.w, ax, bx)));
    return q <= 1.0f;
}
template <bool SLABS = true>
__device__ GSRT_INLINE bool fp_meets(const float4* fps, uint32_t gid, const TileRect& r) {
    const float4* rec = fps + kFpWords * (size_t)gid;
    const float4 box = rec[0];
    const float x0 = r.x0 + kFpInset, x1 = r.x1 - kFpInset, y0 = r.y0 + kFpInset, y1 = r.y1 - kFpInset;
    if (!(box.x <= x1 && box.y >= x0 && box.z <= y1 && box.w >= y0)) return false;
    if (!SLABS) return true;
    const float4 e0 = rec[1], e1 = rec[2];
    return ell_meets(e0, e1, x0, x1, y0, y1);
}

// A super-group's BVH frontier (k_frontier: count, then at most kFront = 128 node refs) held in registers:
// lane l has entries l and 64 + l. The group-list kernel loads it all at once, one memory latency
// instead of two dependent ones (count, then entries). n = kNoGroup: start at the root.
struct FrontRegs { uint32_t n = kNoGroup; uint32_t a = 0u, b = 0u; };
static_assert(kFront <= 128, "FrontRegs holds two entries per lane");

// total: leaves passing the frustum test with key > lo; more: some such leaf (that the cull kept) is not in
// keys[0..count), so another round after keys[count-1] is needed
// n: keys held in the buffer (collect<REGSORT>: unsorted; its caller sorts them and keeps count = min(n, CAP))
struct Collected { uint32_t total; uint32_t count; bool restart; bool more; uint32_t n; bool sorted; };

// COR: compact keys[begin..count) in place (from begin) to the candidates that can contribute to some ray
// of the tile: those whose conservative footprint box (k_project: where g <= min(5.6, ln(255 op)), i.e.
// alpha > 1/255 is possible) meets the tile's sample rectangle. The others have alpha 0 for every ray of the
// tile, so dropping them changes nothing (results stay bit-identical); the shading loop just skips them.
// B chunks of 64 keys per round: their footprint boxes are loaded together (B independent loads per lane in
// flight, one memory latency per round instead of one per chunk); the group lists use B = 4, the render kernel's
// rare own traversal B = 1 (VGPR budget). In place: a round's keys are all read before its first write, and the
// writes land below the next round's keys.
template <uint32_t B = 1>
__device__ GSRT_INLINE uint32_t cull_footprints(uint64_t* keys, uint32_t begin, uint32_t count, const TileRect& rect) {
    const float4* fps = kargs().a.footprint;
    const uint32_t lane = lane_id();
    const float x0 = rect.x0 + kFpInset, x1 = rect.x1 - kFpInset, y0 = rect.y0 + kFpInset, y1 = rect.y1 - kFpInset;
    uint32_t out = begin;
    for (uint32_t base = begin; base < count; base += 64 * B) {
        uint64_t key[B];
        float4 box[B];
#pragma unroll
        for (uint32_t j = 0; j < B; ++j) {
            const uint32_t i = base + 64 * j + lane;
            key[j] = i < count ? keys[i] : 0ull;
        }
#pragma unroll
        for (uint32_t j = 0; j < B; ++j) {
            const uint32_t i = base + 64 * j + lane;
            box[j] = i < count ? fps[kFpWords * (size_t)(uint32_t)key[j]] : make_float4(INFINITY, -INFINITY, INFINITY, -INFINITY);
        }
#pragma unroll
        for (uint32_t j = 0; j < B; ++j) {
            // the box only (fp_meets<false>): a coarse cull on the traversal rect
            const bool keep = box[j].x <= x1 && box[j].y >= x0 && box[j].z <= y1 && box[j].w >= y0;
            const uint64_t b = __ballot(keep);
            if (keep) keys[out + popc_below(b)] = key[j];
            out += (uint32_t)__popcll(b);
        }
    }
    __syncthreads();
    return out;
}

// Gather the keys of every leaf whose box meets the frustum of rect and whose key > lo (when has_lo), keep
// the CAP smallest sorted in keys[0..count) (keys holds 2*CAP). width = nodes popped per step (64; 1 = plain
// DFS whose stack is bounded by the tree depth, used after the LDS stack of stack_limit entries ran out).
// cull: drop leaves whose 2D footprint misses rect (cull_footprints) before the buffer is truncated, so the
// CAP slots hold only splats that can contribute.
// depth_cull (COR keys, not the counting pass): once the buffer has overflowed (keys beyond the CAP nearest exist, so the
// list is `more` already), an internal child whose box's depth bound (depth_lo) lies beyond the current threshold's depth
// holds only keys the final CAP nearest cannot contain, and is not descended into: a volume's far side is not walked.
// MERGE (k_group_list): an overflowed buffer merges its new keys into its sorted CAP (merge_tail) instead of sorting
// all of it again; the render kernel's rare traversals keep the plain sort (the merge's registers spill there)
template <uint32_t CAP, uint32_t BUF, class KeyFn, bool REGSORT = false, bool MERGE = false>
__device__ GSRT_INLINE Collected collect(const TileRect& rect, uint64_t lo, bool has_lo, uint64_t* keys, uint32_t* stack,
                             uint32_t stack_limit, uint32_t width, KeyFn keyfn, bool cull,
                             const FrontRegs& front = FrontRegs{}, bool depth_cull = false) {
    const KArgs& K = kargs();
    const uint32_t lane = lane_id();
    Collected res{0u, 0u, false, false};
    const uint32_t n = K.a.n;
    if (n == 0) return res;
    const BvhNode* nodes = K.a.nodes;
    const SplatRec* recs = K.a.recs;
    const uint32_t root_ref = K.a.root_ref;
    const Frustum F = make_frustum(K.ubo, rect.x0, rect.y0, rect.x1, rect.y1);
    // COR frames with leaf_fp: a leaf passes when its footprint box meets the rectangle (the cull_footprints test,
    // done here on the box the node already holds), so no footprint cull follows
    const bool leaf_fp = K.a.leaf_fp != 0;
    if (leaf_fp) cull = false;
    const float fx0 = rect.x0 + kFpInset, fx1 = rect.x1 - kFpInset, fy0 = rect.y0 + kFpInset, fy1 = rect.y1 - kFpInset;
    uint32_t count = 0, total = 0, sp = 0, culled = 0;  // keys[0..culled) already passed the cull
    uint32_t sorted_n = 0;  // keys[0..sorted_n) sorted: 0, or CAP once the buffer has overflowed
    uint64_t thresh = ~0ull;
    if (!KeyFn::kUsesDepth || !K.a.depth_cull || (K.a.depth_unsafe && *K.a.depth_unsafe)) depth_cull = false;
    const ZRow zr = zrow_of(K.ubo.model_view);
    float tdepth = INFINITY;  // the depth of thresh (finite once the buffer has overflowed)
    bool more = false;
    const uint32_t nfront = front.n;
    if (nfront != kNoGroup && 2 * nfront + 2 <= stack_limit) {
        // start below the root: a frontier of a region containing rect (every node rect's rays can reach)
        if (lane < nfront) stack[lane] = front.a;
        if (64 + lane < nfront) stack[64 + lane] = front.b;
        sp = nfront;
    } else {
        const float rlo[3] = {K.a.root_box[0], K.a.root_box[1], K.a.root_box[2]};
        const float rhi[3] = {K.a.root_box[3], K.a.root_box[4], K.a.root_box[5]};
        if (!box_outside(F, rlo, rhi)) {
            if (root_ref & kLeafBit) {  // single-Gaussian scene: the root is a leaf, its key is in the record
                uint64_t key;
                const uint32_t gid = root_ref & ~kLeafBit;
                if (keyfn(__float_as_uint(recs[gid].depth), gid, key) && (!has_lo || key > lo)) {
                    total = 1;
                    if (lane == 0) keys[0] = key;
                    count = 1;
                }
            } else {
                if (lane == 0) stack[0] = root_ref;
                sp = 1;
            }
        }
    }
    __syncthreads();
#ifdef GSRT_DIAG  // diagnostic build only: traversal vs final cull+sort cycles, steps, popped nodes
    const unsigned long long dg0 = __builtin_amdgcn_s_memtime();
    unsigned long long dg_steps = 0, dg_nodes = 0;
#endif
    while (sp > 0) {
        uint32_t k = sp < width ? sp : width;
        if (sp + k > stack_limit) {  // each popped node pushes at most 2: keep sp - k + 2k <= limit
            k = sp < stack_limit ? stack_limit - sp : 0u;
            if (k == 0) { res.restart = true; break; }
        }
        if (count + 2 * k > BUF) {
            if (cull) {
                count = cull_footprints<REGSORT ? 4u : 1u>(keys, culled, count, rect);
                culled = count;
            }
            if (count + 2 * k > BUF) {  // keep the CAP nearest, tighten the threshold (the LDS sort)
                // after the first overflow keys[0..CAP) is sorted: merge the new keys in (merge_tail) instead of sorting
                // the whole buffer again (a deep frustum overflows every BUF - CAP keys). A footprint cull compacts the
                // sorted part too, so with one the buffer is sorted whole
                if (MERGE && sorted_n == CAP && !cull) merge_tail<BUF, CAP>(keys, count);
                else wave_sort<false>(keys, count);
                sorted_n = CAP;
                more = more || count > CAP;
                count = CAP;
                if (culled > count) culled = count;
                thresh = keys[CAP - 1];
                tdepth = __uint_as_float((uint32_t)(thresh >> 32));
            }
        }
#ifdef GSRT_DIAG
        ++dg_steps;
        dg_nodes += k;
#endif
        const bool act = lane < k;
        const uint32_t node = act ? stack[sp - k + lane] : 0u;
        __syncthreads();
        sp -= k;
        uint32_t np = 0, na = 0, nt = 0, nr = 0;
        uint32_t p0 = 0, p1 = 0;
        uint64_t a0 = 0, a1 = 0;
        if (act) {
            const BvhNode nd = nodes[node];
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const float* clo = side ? nd.r_lo : nd.l_lo;
                const float* chi = side ? nd.r_hi : nd.l_hi;
                const uint32_t ref = side ? nd.r_ref : nd.l_ref;
                if (leaf_fp && (ref & kLeafBit)) {  // the leaf's footprint box {x0, x1, y0, y1} (put_node_key_fp)
                    if (!(clo[0] <= fx1 && clo[1] >= fx0 && clo[2] <= fy1 && chi[0] >= fy0)) continue;
                } else if (box_outside(F, clo, chi)) {
                    continue;
                }
                if (ref & kLeafBit) {
                    uint64_t key;
                    if (keyfn(side ? nd.r_key : nd.l_key, ref & ~kLeafBit, key) && (!has_lo || key > lo)) {
                        ++nt;
                        if (key < thresh) { if (na == 0) a0 = key; else a1 = key; ++na; }
                        else nr = 1;
                    }
                } else if (!(depth_cull && depth_lo(zr, clo, chi) > tdepth)) {
                    if (np == 0) p0 = ref; else p1 = ref;
                    ++np;
                }
            }
        }
        uint64_t b1 = __ballot(np >= 1), b2 = __ballot(np >= 2);
        uint32_t off = popc_below(b1) + popc_below(b2);
        if (np >= 1) stack[sp + off] = p0;
        if (np >= 2) stack[sp + off + 1] = p1;
        sp += (uint32_t)__popcll(b1) + (uint32_t)__popcll(b2);
        b1 = __ballot(na >= 1); b2 = __ballot(na >= 2);
        off = popc_below(b1) + popc_below(b2);
        if (na >= 1) keys[count + off] = a0;
        if (na >= 2) keys[count + off + 1] = a1;
        count += (uint32_t)__popcll(b1) + (uint32_t)__popcll(b2);
        total += (uint32_t)__popcll(__ballot(nt >= 1)) + (uint32_t)__popcll(__ballot(nt >= 2));
        more = more || __ballot(nr != 0) != 0;  // a leaf beyond the threshold: it belongs to a later round
        __syncthreads();
    }
    if (res.restart) return res;
#ifdef GSRT_DIAG
    const unsigned long long dg1 = __builtin_amdgcn_s_memtime();
#endif
    if (cull) count = cull_footprints<REGSORT ? 4u : 1u>(keys, culled, count, rect);
    // REGSORT: the caller sorts keys[0..n) in registers (one inlined copy of the large register network per kernel);
    // the count and the continuation flag below are those of the sorted, truncated list either way. An overflowed
    // buffer (its first CAP keys sorted, no cull) merges its tail in here instead
    res.sorted = MERGE && sorted_n == CAP && !cull;
    if constexpr (MERGE) {
        if (res.sorted) merge_tail<BUF, CAP>(keys, count);
    }
    if (!res.sorted && !REGSORT) wave_sort<false>(keys, count);
#ifdef GSRT_DIAG
    if (lane == 0) {
        atomicAdd(K.a.counters + 12, dg1 - dg0);
        atomicAdd(K.a.counters + 13, __builtin_amdgcn_s_memtime() - dg1);
        atomicAdd(K.a.counters + 14, dg_steps);
        atomicAdd(K.a.counters + 15, dg_nodes);
    }
#endif
    res.total = total;
    res.more = more || count > CAP;
    res.count = count < CAP ? count : CAP;
    res.n = count;
    return res;
}

template <uint32_t CAP = kCap, uint32_t BUF = 2 * CAP, class KeyFn, bool REGSORT = false, bool MERGE = false>
__device__ GSRT_INLINE Collected collect_robust(const TileRect& rect, uint64_t lo, bool has_lo, uint64_t* keys,
                                           uint32_t* stack, KeyFn keyfn, uint32_t& restarts, bool cull = false,
                                           uint32_t stack_limit = 0, const FrontRegs& front = FrontRegs{},
                                           bool depth_cull = false) {
    if (!stack_limit) stack_limit = kargs().a.stack_limit;
    static_assert((BUF & (BUF - 1)) == 0 && BUF >= CAP + 128, "keys buffer: a power of two (wave_sort pads to one) with room for a step");
    // a 64-wide packet walk, and after a stack overflow the one-node-wide DFS
    Collected c;
    if constexpr (MERGE) {  // (one inlined copy of collect for both widths: the group-list kernel stays compact)
        for (uint32_t width = 64u;; width = 1u) {
            c = collect<CAP, BUF, KeyFn, REGSORT, MERGE>(rect, lo, has_lo, keys, stack, stack_limit, width, keyfn, cull,
                                                         front, depth_cull);
            if (!c.restart || width == 1u) break;
            ++restarts;
            __syncthreads();
        }
    } else {
        c = collect<CAP, BUF, KeyFn, REGSORT, MERGE>(rect, lo, has_lo, keys, stack, stack_limit, 64u, keyfn, cull, front,
                                                     depth_cull);
        if (c.restart) {
            ++restarts;
            __syncthreads();
            c = collect<CAP, BUF, KeyFn, REGSORT, MERGE>(rect, lo, has_lo, keys, stack, stack_limit, 1u, keyfn, cull, front,
                                                         depth_cull);
        }
    }
    if (c.restart && lane_id() == 0) atomicOr(kargs().a.counters + kErrWord, 1ull);
    if (REGSORT && !c.restart && !c.sorted) wave_sort<true>(keys, c.n);  // the one register-sort site of the kernel
    return c;
}

__device__ GSRT_INLINE void add_counters(unsigned long long rays, unsigned long long cand, unsigned long long blended,
                                    unsigned long long term, unsigned long long rounds, unsigned long long restarts,
                                    unsigned long long maxc) {
    if (lane_id() != 0) return;
    unsigned long long* c = kargs().a.counters;
    atomicAdd(c + 0, rays);
    atomicAdd(c + 1, cand);
    atomicAdd(c + 2, blended);
    atomicAdd(c + 3, term);
    atomicAdd(c + 4, rounds);
    atomicAdd(c + 5, restarts);
    atomicAdd(c + 6, 1ull);
    atomicMax(c + 7, maxc);
}

// ----------------------------------------------------------------------------------------- COR

// LDS stage of one group of sorted candidates: the 64-B records and the SH-3 coefficients. Filled by LDS-DMA
// (global_load_lds, 16 B per lane, no VGPR destination): the stage is 16-B pieces in lane order, records first.
// A kind whose output has its own table (feat: 64-B feature rows) stages its rows at the start of sh, and no SH rows.
struct Stage {
    SplatRec rec[kGroup];         // kGroup * 64 B
    float sh[kGroup][3][16];      // kGroup * 192 B, device layout [gauss][rgb][coef]
};
static_assert(sizeof(Stage) == kGroup * 256 && sizeof(Stage) % 1024 == 0, "whole wave-instructions of 16-B pieces");

// The wait for the stage issued `younger` stages before the most recent one: vmcnt counts VMEM operations in issue
// order, so vmcnt(younger * stage_ops) leaves the younger stages' DMAs in flight (any other younger VMEM operation only
// makes the wait stricter)
template <uint32_t N>
__device__ GSRT_INLINE void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <class V>
__device__ GSRT_INLINE void wait_stage(uint32_t younger) {
    constexpr uint32_t P = V::stage_ops;
    if (younger >= 2) wait_vmcnt<2 * P>();
    else if (younger == 1) wait_vmcnt<P>();
    else wait_vmcnt<0>();
}

// A read of LDS that no LDS-DMA in flight writes (the round's id list, complete before shading starts), hidden from
// the compiler's LDS-DMA tracking: a plain read of it after a stage's DMA makes the compiler wait for vmcnt(0), i.e.
// for every stage in flight, which would leave the stage pipeline one stage deep. The value is waited for here.
__device__ GSRT_INLINE uint32_t lds_read_settled(const uint32_t* p) {
    const uint32_t a = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t*)p;
    uint32_t v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
    return v;
}

// issue the LDS-DMA of group g0 of ids[0..count) into dst: piece p < 4*kGroup is quarter p&3 of record p>>2,
// the next 12*kGroup pieces are the SH rows (12 pieces each); piece p lands at byte 16 p of the stage. Every
// lane computes its piece's address the same way (base, row stride and offset selected, no divergent paths).
// Waited for by wait_stage before the stage is read. sh is the output's table (Out::rows): feat's row is 4 pieces
// (64 B), so its stage is 4 kGroup record pieces and 4 kGroup feature pieces, one DMA instruction.
template <class V>
__device__ GSRT_INLINE void stage_issue(const uint32_t* ids, uint32_t count, uint32_t g0, uint32_t lane, Stage* dst,
                                   const SplatRec* recs, const float* sh) {
    constexpr uint32_t kRecPieces = 4 * kGroup, kPieces = V::stage_pieces, kRowPieces = V::row_pieces;
#pragma unroll
    for (uint32_t i = 0; i < (kPieces + 63) / 64; ++i) {
        const uint32_t p = i * 64 + lane;
        const bool is_rec = p < kRecPieces;
        const uint32_t q = p - kRecPieces;
        uint32_t c = g0 + (is_rec ? p >> 2 : q / kRowPieces);
        c = c < count ? c : g0;  // past the list's end: a copy of candidate g0 (never read; keeps lane 0 active)
        if (p < kPieces) {       // lane 0 always loads: each stage is exactly stage_ops DMA instructions
            const uint32_t id = lds_read_settled(ids + c);
            const char* base = is_rec ? reinterpret_cast<const char*>(recs) : reinterpret_cast<const char*>(sh);
            const uint32_t stride = is_rec ? 64u : kRowPieces * 16u, off = is_rec ? (p & 3) * 16u : (q % kRowPieces) * 16u;
            __builtin_amdgcn_global_load_lds((const void*)(base + (size_t)id * stride + off),
                                             (void*)(reinterpret_cast<char*>(dst) + i * 1024), 16, 0, 0);
        }
    }
}

// and its first 128 ids into ids[0..128) (waited for by the next vmcnt(0), i.e. __syncthreads)
__device__ GSRT_INLINE void list_issue(uint32_t lt, uint32_t lane, uint32_t* ids, uint32_t* hdr) {
    const KArgs& K = kargs();
    const uint32_t* src = K.a.lists + (size_t)lt * kCap;
    __builtin_amdgcn_global_load_lds((const void*)(src + lane), (void*)ids, 4, 0, 0);
    __builtin_amdgcn_global_load_lds((const void*)(src + 64 + lane), (void*)(ids + 64), 4, 0, 0);
    if (lane < 4)
        __builtin_amdgcn_global_load_lds((const void*)(reinterpret_cast<const uint32_t*>(K.a.list_hdr + lt) + lane),
                                         (void*)hdr, 4, 0, 0);
}

template <class V>
struct CorRay {
    ObjRay R;
    float pxs, pys;
    float bs[16];
    float T, C[3];
    typename V::RayPayload k;  // the kind's own: its output's sums (feat: no bs there) or its sink's payload
    bool active;
    uint32_t cand, blended, term;
#ifdef GSRT_DIAG
    // wave-candidates (per wave, lane 0 adds): staged while some lane active; some lane passed g; some lane's
    // alpha > 0; some lane blended (SH evaluated); lane-candidates passing g; lane blends
    uint32_t dg_staged, dg_gpass, dg_contrib, dg_blend, dg_lanes_g, dg_lanes_blend;
    // stages shaded while some lane active; of those, stages some lane blends in; over those, the sum of the largest
    // number of candidates one lane blends (dg_blend counts blend_hit's). The SH colour kinds (shade_lanes) count
    // passes instead: stages some lane passes g in, the passes run, and in dg_lanes_g / dg_lanes_blend the lanes of a pass
    // and those of them that blend; dg_gpass, dg_contrib and dg_blend stay 0 there
    uint32_t dg_stages, dg_stages_blend, dg_lane_max;
    // over the stages shaded: the candidates some lane passes g on, and the largest number of candidates one lane passes
    // g on (both from the okg ballots after phase 1, before any stop clears a lane)
    uint32_t dg_g_any, dg_g_lane_max;
#endif
};

// Front-to-back blend of candidate c (alpha 0: no contribution) into every lane's ray; the SH-3 colour only
// when some lane blends. A ray whose transmittance would drop below 1e-4 stops (the hit is not blended):
// returns the mask of the lanes whose ray stopped here. contrib is the wave's lane mask of alpha > 0: the masks are
// ballots combined by scalar instructions (SGPR pairs), read back per lane by lane_of.
// channel colour 0.5 + sum basis * coef (the 0.5 and s_0 Y_0 folded into coefficient 0, gsrt_api.cpp upload_common),
// clamped at 0: the same fma chain whatever the coefficients' home
__device__ GSRT_INLINE float sh_channel(const float (&bs)[16], const float (&s)[16]) {
    float a = s[0];
#pragma unroll
    for (int q = 1; q < 16; ++q) a = fmaf(bs[q], s[q], a);
    return a > 0.0f ? a : 0.0f;
}
// the stage's LDS copy of candidate c's row. c is wave-uniform (broadcast reads) or the lane's own (lane_pass): the
// stage's rows lie 192 B = 48 banks apart, so lanes reading the same 16-B piece of different rows meet four distinct
// 4-bank groups, and a ds_read_b128 costs its 4 LDS-array cycles either way
struct ShFromStage {
    const Stage* stg;
    uint32_t c;
    __device__ GSRT_INLINE void operator()(const float (&bs)[16], float (&col)[3]) const {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float4* s4 = reinterpret_cast<const float4*>(stg->sh[c][ch]);
            const float4 q0 = s4[0], q1 = s4[1], q2 = s4[2], q3 = s4[3];
            const float s[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                                 q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
            col[ch] = sh_channel(bs, s);
        }
    }
};
// This lane's bit of a wave-uniform lane mask (a ballot held in an SGPR pair): the mask itself is the v_cndmask
// or exec source, no compare forms it again.
__device__ GSRT_INLINE bool lane_of(uint64_t mask) { return __builtin_amdgcn_inverse_ballot_w64(mask); }
// GRAD: the sums of t[0..16) over the lanes of each 16-lane row, transposed: lane l returns the sum of t[l & 15] over
// its row. A butterfly that halves the channels a lane carries at every step: partners 15 - i (row_mirror), 7 - i within
// 8 lanes (row_half_mirror), i ^ 2 and i ^ 1 (quad permutes). A lane keeps the half its own lane bit names and sends
// the other half, which is the half its partner keeps: 8 + 4 + 2 + 1 = 15 DPP moves instead of 16 x 4 for one
// reduction per channel. The four partner sets of a lane tile its row, so every lane's term enters each sum once.
template <int CTRL>
__device__ GSRT_INLINE float dpp_from(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ GSRT_INLINE float grad_row_sums(const float (&t)[16]) {
    const bool b3 = lane_of(0xFF00FF00FF00FF00ull), b2 = lane_of(0xF0F0F0F0F0F0F0F0ull);
    const bool b1 = lane_of(0xCCCCCCCCCCCCCCCCull), b0 = lane_of(0xAAAAAAAAAAAAAAAAull);
    float a[8], b[4], c[2];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = (b3 ? t[8 + k] : t[k]) + dpp_from<0x140>(b3 ? t[k] : t[8 + k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = (b2 ? a[4 + k] : a[k]) + dpp_from<0x141>(b2 ? a[k] : a[4 + k]);
#pragma unroll
    for (int k = 0; k < 2; ++k) c[k] = (b1 ? b[2 + k] : b[k]) + dpp_from<0x4E>(b1 ? b[k] : b[2 + k]);
    return (b0 ? c[1] : c[0]) + dpp_from<0xB1>(b0 ? c[0] : c[1]);
}
// GRAD: a stage's four row sums per lane (gs[c]: candidate c, channel l & 15, the lane's 16-lane row) to the wave's sums,
// transposed once more: lane 16 c + ch returns the wave's sum of candidate c's channel ch. v_permlane32_swap exchanges
// the upper 32 lanes of its first operand with the lower 32 of its second, v_permlane16_swap the odd 16-lane rows of the
// first with the even rows of the second: after either, first + second holds the first operand's sum on the lanes
// that kept it and the second's on the others. Three swaps and three adds.
__device__ GSRT_INLINE float grad_stage_sums(const float (&gs)[kGroup]) {
    static_assert(kGroup == 4, "one candidate per 16-lane row");
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 p = __builtin_amdgcn_permlane32_swap(__float_as_uint(gs[0]), __float_as_uint(gs[2]), false, false);
    const u32x2 q = __builtin_amdgcn_permlane32_swap(__float_as_uint(gs[1]), __float_as_uint(gs[3]), false, false);
    const float u = __uint_as_float(p.x) + __uint_as_float(p.y);  // candidate 0 on lanes 0..31, candidate 2 above
    const float v = __uint_as_float(q.x) + __uint_as_float(q.y);  // candidates 1 and 3
    const u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(u), __float_as_uint(v), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
// opgrad: a stage's four terms per lane (t[c]: candidate c) to the wave's sums, transposed: every lane l returns the wave's
// sum of candidate l & 3. Inside a quad the butterfly of grad_row_sums' last two steps (partners i ^ 2 and i ^ 1: a lane
// keeps the half its own lane bit names and sends the other), then the four quads of a row by two row rotations, which
// keep l & 3, and the four rows by the two permlane swaps of a value with itself (grad_stage_sums): first + second
// is then the sum of both halves on every lane.
__device__ GSRT_INLINE float opgrad_stage_sums(const float (&t)[kGroup]) {
    static_assert(kGroup == 4, "one candidate per lane of a quad");
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    const bool b1 = lane_of(0xCCCCCCCCCCCCCCCCull), b0 = lane_of(0xAAAAAAAAAAAAAAAAull);
    float c[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) c[k] = (b1 ? t[2 + k] : t[k]) + dpp_from<0x4E>(b1 ? t[k] : t[2 + k]);
    float v = (b0 ? c[1] : c[0]) + dpp_from<0xB1>(b0 ? c[0] : c[1]);  // the quad's sum of candidate l & 3
    v = v + dpp_from<0x128>(v);  // row_ror:8
    v = v + dpp_from<0x124>(v);  // row_ror:4: the row's sum
    const u32x2 p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const float u = __uint_as_float(p.x) + __uint_as_float(p.y);  // rows 0 + 1 below lane 32, rows 2 + 3 above
    const u32x2 q = __builtin_amdgcn_permlane32_swap(__float_as_uint(u), __float_as_uint(u), false, false);
    return __uint_as_float(q.x) + __uint_as_float(q.y);
}
// x summed over ns samples to their mean: x * (1 / ns) for a power of two (x / 2^k == x * 2^-k exactly), else x / ns
__device__ GSRT_INLINE float over_samples(float x, uint32_t ns) {
    const float nsf = (float)ns;
    return (ns & (ns - 1)) == 0 ? x * (1.0f / nsf) : x / nsf;
}

// ---- gradient sinks. A gradient frame is the backward of a forward frame to one per-Gaussian table (RenderArgs::grad_in,
// grad_rows). What its kind adds to the shading loop is one type, its sink; the loop (shade_sorted, shade_stage,
// blend_hit) names no kind and calls the sink it is given. A sink holds where a round's terms go (of_frame) and supplies
//   Payload, load: the lane's upstream gradient in the ray (CorRay::k) and how it is read;
//   share(ids + g0): one stage's share of the round, a Share: the stage's candidate ids (in the round's list in LDS), the
//     mask of the candidates some lane blended (bit c, wave-uniform) and the kind's sums. shade_stage tells it each
//     candidate's exponential, |opacity| and staged record before the hit (candidate), blend_hit calls hit for the wave where some lane
//     blends candidate c (T still the hit's T_i, col its colour) and hit_lane on the blending lanes once the colour is
//     accumulated, and shade_stage ends with flush where mask is set: the stage's terms, summed over the wave, to the table.
// The lane's upstream gradient of a colour frame: the first N floats of pixel (x, y) of grad_in, an RGBA image, scaled
// once by 1 / ns as the forward store scales the sums; invalid lanes hold +0
template <int N>
__device__ GSRT_INLINE void load_upstream(float (&G)[N], uint32_t x, uint32_t y, bool valid, uint32_t ns) {
    const KArgs& K = kargs();
    const float* gi = K.a.grad_in + ((size_t)y * K.a.width + x) * 4;
#pragma unroll
    for (int q = 0; q < N; ++q) G[q] = valid ? over_samples(gi[q], ns) : 0.0f;
}
// The frame of a flush (shade_stage calls it only where some lane blended in the stage), PER lanes a candidate: the
// wave's sums (sums(), every lane), and lane PER c + off adds (add) for candidate c if some lane blended it. A blended
// candidate c is below the stage's m, so ids[c] is an entry of the round's list: its id is below n, its row in the table.
template <uint32_t PER, class Sums, class Add>
__device__ GSRT_INLINE void flush_share(const uint32_t* ids, uint32_t mask, Sums sums, Add add) {
    const auto sum = sums();
    const uint32_t l = lane_here(), c = l / PER, off = l % PER;
    if ((PER * kGroup == 64 || c < kGroup) && ((mask >> c) & 1u)) add(lds_read_settled(ids + c), off, sum);
}
// No gradient: plain, stats, depth and feat frames, and the first sweep of an opgrad kernel
struct NoGrad {
    __device__ GSRT_INLINE static NoGrad of_frame() { return {}; }
    struct Payload {};
    template <class P> __device__ GSRT_INLINE static void load(P&, uint32_t, uint32_t, bool, uint32_t) {}
    struct Share {
        static constexpr uint32_t mask = 0;  // never a flush
        __device__ GSRT_INLINE void candidate(float, float, const SplatRec*) {}
        template <class Ray> __device__ GSRT_INLINE void hit(uint32_t, uint64_t, float, const float (&)[3], const Ray&) {}
        template <class Ray> __device__ GSRT_INLINE void hit_lane(uint32_t, float, const float (&)[3], const Ray&) {}
        __device__ GSRT_INLINE void flush() const {}
    };
    __device__ GSRT_INLINE Share share(const uint32_t*) const { return {}; }
};
// grad (GSRT_FLAG_FEATURE_GRAD): the backward of a feature frame to the feature table, rows of 16 floats of which
// `channels` are in use; the RGBA is the feature frame's. G_c / ns per channel in the ray. A hit's terms t_c = w G_c of
// the blending lanes (+0, selected, on every other lane) are summed over each 16-lane row into the share's sums
// (grad_row_sums); the flush is one atomic wave-instruction, lane 16 c + ch adding the wave's sum for candidate c and
// channel ch. A/B builds (make ab AB_FLAGS=..., never the product library) set GSRT_GRAD_AB: 1 leaves the atomic out
// (timing only), 2 makes it count adds per row and wave-instructions instead of summing (profiles/feature_grad_cost.py)
struct FeatureGrad {
    float* rows;
    uint32_t channels;  // of a row's 16 floats, the ones in use
    __device__ GSRT_INLINE static FeatureGrad of_frame() { return {kargs().a.grad_rows, kargs().a.grad_channels}; }
    struct Payload { float G[16]; };
    __device__ GSRT_INLINE static void load(Payload& g, uint32_t x, uint32_t y, bool valid, uint32_t ns) {
        const KArgs& K = kargs();  // load_upstream written out, as is the flush below: through the shared helpers the two
        const uint32_t C = K.a.grad_channels;  // kernels' code differed and the 16-channel frame measured 0.3 % slower
        const float* gi = K.a.grad_in + ((size_t)y * K.a.width + x) * C;
#pragma unroll
        for (int q = 0; q < 16; ++q) g.G[q] = valid && (uint32_t)q < C ? over_samples(gi[q], ns) : 0.0f;
    }
    struct Share {
        const uint32_t* ids;
        float* rows;
        uint32_t channels;  // channels from here on (G holds +0 there) are left out
        float sums[kGroup] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t mask = 0;
        __device__ GSRT_INLINE void candidate(float, float, const SplatRec*) {}
        template <class Ray>
        __device__ GSRT_INLINE void hit(uint32_t c, uint64_t blend, float alpha, const float (&)[3], const Ray& ray) {
            const float w = alpha * ray.T;  // the blend's own weight
            const bool mine = lane_of(blend);
            float t[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) t[q] = mine ? w * ray.k.G[q] : 0.0f;  // a select: another lane's G never enters
            sums[c] = grad_row_sums(t);
            mask |= 1u << c;
        }
        template <class Ray> __device__ GSRT_INLINE void hit_lane(uint32_t, float, const float (&)[3], const Ray&) {}
        __device__ GSRT_INLINE void flush() const {
            const float sum = grad_stage_sums(sums);
            const uint32_t l = lane_here(), c = l >> 4, ch = l & 15u;
            if (((mask >> c) & 1u) && ch < channels) {  // flush_share<16> written out
                const uint32_t id = lds_read_settled(ids + c);
#if GSRT_GRAD_AB == 1  // timing only: the reduction without its atomic
                asm volatile("" ::"v"(sum), "v"(id));
#elif GSRT_GRAD_AB == 2  // counting: channel 0 counts the adds a row receives, channel 1 the wave-instructions
                const float one = ch == 0 || c == (uint32_t)__builtin_ctz(mask) ? 1.0f : 0.0f;
                asm volatile("" ::"v"(sum));
                atomicAdd(rows + (size_t)id * 16u + ch, one);
#else
                atomicAdd(rows + (size_t)id * 16u + ch, sum);  // no-return global_atomic_add_f32
#endif
            }
        }
    };
    __device__ GSRT_INLINE Share share(const uint32_t* ids) const { return Share{ids, rows, channels}; }
};
// shgrad (GSRT_FLAG_SH_GRAD): the backward of a plain colour frame to the SH table, rows of 192 B per Gaussian id,
// [rgb][coef] as the SH rows are; SH rows always, and the plain frame's RGBA. The upstream colour gradient G_ch / ns in
// the ray (an RGBA image's first three floats: alpha does not depend on SH). Per colour channel a hit's terms
// t_q = (w G_ch) Y_q of the blending lanes whose channel the clamp let through (col[ch] > 0 exactly when sh_channel's
// chain ended above 0), +0, selected, on every other lane, are summed as grad's are; Y_q is the ray's own basis,
// bs[0] = kShY0: the gradient is with respect to the API's s_0, not the folded word. The flush is three atomic
// wave-instructions, one per colour channel, lane 16 c + q adding coefficient q.
struct ShGrad {
    float* rows;
    __device__ GSRT_INLINE static ShGrad of_frame() { return {kargs().a.grad_rows}; }
    struct Payload { float G[3]; };
    __device__ GSRT_INLINE static void load(Payload& g, uint32_t x, uint32_t y, bool v, uint32_t ns) { load_upstream(g.G, x, y, v, ns); }
    struct Share {
        const uint32_t* ids;
        float* rows;
        float sums[3][kGroup] = {};
        uint32_t mask = 0;
        struct Rgb { float v[3]; };
        __device__ GSRT_INLINE void candidate(float, float, const SplatRec*) {}
        template <class Ray>
        __device__ GSRT_INLINE void hit(uint32_t c, uint64_t blend, float alpha, const float (&col)[3], const Ray& ray) {
            const float w = alpha * ray.T;  // the blend's own weight
            const bool mine = lane_of(blend);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const bool on = mine && col[ch] > 0.0f;
                const float wg = w * ray.k.G[ch];
                float t[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) t[q] = on ? wg * ray.bs[q] : 0.0f;
                sums[ch][c] = grad_row_sums(t);
            }
            mask |= 1u << c;
        }
        template <class Ray> __device__ GSRT_INLINE void hit_lane(uint32_t, float, const float (&)[3], const Ray&) {}
        __device__ GSRT_INLINE void flush() const {
            flush_share<16>(ids, mask, [&] {
                Rgb sum;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) sum.v[ch] = grad_stage_sums(sums[ch]);
                return sum;
            }, [&](uint32_t id, uint32_t q, const Rgb& sum) {
                float* row = rows + (size_t)id * 48u + q;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) atomicAdd(row + 16 * ch, sum.v[ch]);  // no-return global_atomic_add_f32
            });
        }
    };
    __device__ GSRT_INLINE Share share(const uint32_t* ids) const { return Share{ids, rows}; }
};
// What the sinks of the resweep kinds (opgrad, splatgrad) and their Shares derive from. In the ray the upstream gradient
// G_ch / ns of all four channels and the first sweep's finals: the colour C_ch and the transmittance T_end. candidate:
// the hit's exponential e and whether fl(|o| e) < 0.99f, i.e. whether alpha is |o| e and not the clamp's constant.
// dalpha: d = d(frame . G) / d(alpha) of a blended hit, from the finals and the running colour after this hit
struct ResweepGrad {
    struct Payload { float G[4], fin[4]; };
    __device__ GSRT_INLINE static void load(Payload& g, uint32_t x, uint32_t y, bool valid, uint32_t ns) {
        load_upstream(g.G, x, y, valid, ns);
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) g.fin[ch] = 0.0f;  // k_render_cor sets them before the second sweep
    }
    template <class Terms>  // t: the lane's terms of the stage, the sink's own array; before mask as it was: DESIGN.md 3
    struct ShareOf {
        const uint32_t* ids;
        float* rows;
        Terms t = {};
        uint32_t mask = 0; float e = 0.0f; bool open = false;
        __device__ GSRT_INLINE void candidate(float e_, float o, const SplatRec*) { e = e_, open = o * e_ < 0.99f; }
        template <class Ray>
        __device__ GSRT_INLINE void hit(uint32_t c, uint64_t, float, const float (&)[3], const Ray&) { mask |= 1u << c; }
        template <class Ray>
        __device__ GSRT_INLINE float dalpha(float alpha, const float (&col)[3], const Ray& ray) const {
            const float r = 1.0f / (1.0f - alpha);  // alpha <= 0.99
            float d = (ray.k.G[3] * ray.k.fin[3]) * r;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) d = d + ray.k.G[ch] * (ray.T * col[ch] - (ray.k.fin[ch] - ray.C[ch]) * r);
            return d;
        }
    };
};
// opgrad (GSRT_FLAG_OPACITY_GRAD): the backward of a plain colour frame to the opacities (one float per Gaussian id),
// with or without SH rows; the plain frame's RGBA. Every pass shades its rays twice (k_render_cor): the plain blend with
// NoGrad for the ray's finals, then the same blend again with this sink. hit_lane: the hit's d (ResweepGrad) times
// d(alpha) / d|o| = e where the clamp let |o| e through, a select: every other lane keeps the share's +0 in t[c]. The
// flush sums the lanes' terms over the wave (opgrad_stage_sums): one atomic wave-instruction, lane c < kGroup adds.
struct OpacityGrad : ResweepGrad {
    float* rows;
    __device__ GSRT_INLINE static OpacityGrad of_frame() { return {{}, kargs().a.grad_rows}; }
    struct Share : ShareOf<float[kGroup]> {
        template <class Ray>
        __device__ GSRT_INLINE void hit_lane(uint32_t c, float alpha, const float (&col)[3], const Ray& ray) {
            const float d = dalpha(alpha, col, ray);
            t[c] = open ? d * e : 0.0f;
        }
        __device__ GSRT_INLINE void flush() const {
            flush_share<1>(ids, mask, [&] { return opgrad_stage_sums(t); },
                           [&](uint32_t id, uint32_t, float sum) { atomicAdd(rows + id, sum); });
        }
    };
    __device__ GSRT_INLINE Share share(const uint32_t* ids) const { return Share{{ids, rows}}; }
};
// splatgrad (GSRT_FLAG_SPLAT_GRAD): the backward of a plain colour frame to each Gaussian's screen-space splat: the pixel
// centre (ppx, ppy) and the conic (A, B, C) of g = (A dx^2 + 2 B dx dy + C dy^2) / 2, with or without SH rows; the plain
// frame's RGBA. Sweeps as opgrad's: the second forms the same d per blended hit (ResweepGrad). Where the clamp let
// |o| e through, d(alpha) / dg = -alpha, so q = -alpha d weighs dg / d(ppx, ppy, A, B, C); the lane reads the
// candidate's centre and conic again from its staged record (words 8..12; the record stores A / 2 and C / 2, exact
// halves) and forms dx, dy as phase 1 of shade_stage formed them. Slot 5 is opgrad's own term d e. Selects: the lanes
// that do not blend c and the clamped hits keep the share's +0. The flush pads a candidate's six sums to eight and sums
// them over the wave as grad's sixteen channels are: candidates 0, 1 and 2, 3 through grad_row_sums, the rows through
// grad_stage_sums, which leaves candidate c's slot q on lane 8 c + q; one atomic wave-instruction, 24 lanes add.
struct SplatGrad : ResweepGrad {
    float* rows;
    __device__ GSRT_INLINE static SplatGrad of_frame() { return {{}, kargs().a.grad_rows}; }
    static constexpr uint32_t kSlots = 6;  // of a row's 8 floats, the ones a frame adds to
    struct Share : ShareOf<float[kGroup][kSlots]> {
        const SplatRec* rec = nullptr;
        __device__ GSRT_INLINE void candidate(float e_, float o, const SplatRec* r) { ShareOf::candidate(e_, o, r), rec = r; }
        template <class Ray>
        __device__ GSRT_INLINE void hit_lane(uint32_t c, float alpha, const float (&col)[3], const Ray& ray) {
            const float d = dalpha(alpha, col, ray);
            const float4 q2 = reinterpret_cast<const float4*>(rec)[2];  // ppx, ppy, A/2, B
            const float4 q3 = reinterpret_cast<const float4*>(rec)[3];  // C/2, ...
            const float dx = ray.pxs - q2.x, dy = ray.pys - q2.y;       // the blending lanes' rays are live: no NaN
            const float A = 2.0f * q2.z, B = q2.w, C = 2.0f * q3.x;
            const float q = -(alpha * d);
            t[c][0] = open ? q * -(A * dx + B * dy) : 0.0f;
            t[c][1] = open ? q * -(B * dx + C * dy) : 0.0f;
            t[c][2] = open ? q * (0.5f * (dx * dx)) : 0.0f;
            t[c][3] = open ? q * (dx * dy) : 0.0f;
            t[c][4] = open ? q * (0.5f * (dy * dy)) : 0.0f;
            t[c][5] = open ? d * e : 0.0f;
        }
        __device__ GSRT_INLINE void flush() const {
            static_assert(kGroup == 4 && kSlots <= 8, "two candidates of eight slots per grad_row_sums");
            flush_share<8>(ids, mask, [&] {
                float lo[16], hi[16];
#pragma unroll
                for (uint32_t q = 0; q < 8; ++q) {
                    lo[q] = q < kSlots ? t[0][q] : 0.0f, lo[8 + q] = q < kSlots ? t[1][q] : 0.0f;
                    hi[q] = q < kSlots ? t[2][q] : 0.0f, hi[8 + q] = q < kSlots ? t[3][q] : 0.0f;
                }
                const float gs[kGroup] = {grad_row_sums(lo), grad_row_sums(hi), 0.0f, 0.0f};
                return grad_stage_sums(gs);  // lanes 0..15: candidates 0, 1; lanes 16..31: candidates 2, 3
            }, [&](uint32_t id, uint32_t q, float sum) {
                if (q < kSlots) atomicAdd(rows + (size_t)id * 8u + q, sum);  // no-return global_atomic_add_f32
            });
        }
    };
    __device__ GSRT_INLINE Share share(const uint32_t* ids) const { return Share{{ids, rows}}; }
};
// splatdepthgrad (GSRT_FLAG_SPLAT_DEPTH_GRAD): the backward of a depth frame, RGBA and D = sum z w together, to the splat
// rows; the plain frame's RGBA. Depth is one more blended channel whose colour is the hit's own z, the staged record's
// view depth (word 3: the value DepthOut::blend takes and the hits are keyed by). In the ray, beside ResweepGrad's
// payload: Gd, the depth image's upstream gradient over ns, the first sweep's final D (finD) and the running D, which both
// sweeps form as the depth frame does (fma(z, w, D) from +0). The first sweep runs with Finals, whose hit_lane adds to D
// and nothing else; the second forms d as splatgrad does plus Gd (T z - (finD - Dafter) r), r the reciprocal of 1 - alpha
// that dalpha divides by, and slots 0..5 from that d with splatgrad's own formulas. Slot 6 is dL/dz = w Gd on every
// blending lane, clamped alpha or not: dD/dz = w does not pass through the clamp. The flush is SplatGrad's with seven
// slots: 28 lanes add.
struct SplatDepthGrad : ResweepGrad {
    float* rows;
    __device__ GSRT_INLINE static SplatDepthGrad of_frame() { return {{}, kargs().a.grad_rows}; }
    struct Payload { float G[4], Gd, fin[4], finD, D; };
    __device__ GSRT_INLINE static void load(Payload& g, uint32_t x, uint32_t y, bool valid, uint32_t ns) {
        load_upstream(g.G, x, y, valid, ns);
        const KArgs& K = kargs();
        g.Gd = valid ? over_samples(K.a.grad_depth_in[(size_t)y * K.a.width + x], ns) : 0.0f;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) g.fin[ch] = 0.0f;  // k_render_cor sets them, and finD, before the second sweep
        g.finD = 0.0f, g.D = 0.0f;
    }
    // the first sweep's sink: the plain blend (no terms, never a flush) that also leaves the ray's D
    struct Finals {
        struct Share {
            static constexpr uint32_t mask = 0;
            const SplatRec* rec = nullptr;
            __device__ GSRT_INLINE void candidate(float, float, const SplatRec* r) { rec = r; }
            template <class Ray> __device__ GSRT_INLINE void hit(uint32_t, uint64_t, float, const float (&)[3], const Ray&) {}
            template <class Ray> __device__ GSRT_INLINE void hit_lane(uint32_t, float alpha, const float (&)[3], Ray& ray) {
                ray.k.D = fmaf(rec->depth, alpha * ray.T, ray.k.D);
            }
            __device__ GSRT_INLINE void flush() const {}
        };
        __device__ GSRT_INLINE Share share(const uint32_t*) const { return {}; }
    };
    static constexpr uint32_t kSlots = 7;  // of a row's 8 floats, the ones a frame adds to
    struct Share : ShareOf<float[kGroup][kSlots]> {
        const SplatRec* rec = nullptr;
        __device__ GSRT_INLINE void candidate(float e_, float o, const SplatRec* r) { ShareOf::candidate(e_, o, r), rec = r; }
        template <class Ray>
        __device__ GSRT_INLINE void hit_lane(uint32_t c, float alpha, const float (&col)[3], Ray& ray) {
            const float z = rec->depth;
            const float w = alpha * ray.T;  // the blend's own weight
            ray.k.D = fmaf(z, w, ray.k.D);  // Dafter_i
            const float r = 1.0f / (1.0f - alpha);  // dalpha's own
            const float d = dalpha(alpha, col, ray) + ray.k.Gd * (ray.T * z - (ray.k.finD - ray.k.D) * r);
            const float4 q2 = reinterpret_cast<const float4*>(rec)[2];  // ppx, ppy, A/2, B
            const float4 q3 = reinterpret_cast<const float4*>(rec)[3];  // C/2, ...
            const float dx = ray.pxs - q2.x, dy = ray.pys - q2.y;       // the blending lanes' rays are live: no NaN
            const float A = 2.0f * q2.z, B = q2.w, C = 2.0f * q3.x;
            const float q = -(alpha * d);
            t[c][0] = open ? q * -(A * dx + B * dy) : 0.0f;
            t[c][1] = open ? q * -(B * dx + C * dy) : 0.0f;
            t[c][2] = open ? q * (0.5f * (dx * dx)) : 0.0f;
            t[c][3] = open ? q * (dx * dy) : 0.0f;
            t[c][4] = open ? q * (0.5f * (dy * dy)) : 0.0f;
            t[c][5] = open ? d * e : 0.0f;
            t[c][6] = w * ray.k.Gd;  // only the blending lanes get here: every other lane keeps the share's +0
        }
        __device__ GSRT_INLINE void flush() const {
            static_assert(kGroup == 4 && kSlots <= 8, "two candidates of eight slots per grad_row_sums");
            flush_share<8>(ids, mask, [&] {
                float lo[16], hi[16];
#pragma unroll
                for (uint32_t q = 0; q < 8; ++q) {
                    lo[q] = q < kSlots ? t[0][q] : 0.0f, lo[8 + q] = q < kSlots ? t[1][q] : 0.0f;
                    hi[q] = q < kSlots ? t[2][q] : 0.0f, hi[8 + q] = q < kSlots ? t[3][q] : 0.0f;
                }
                const float gs[kGroup] = {grad_row_sums(lo), grad_row_sums(hi), 0.0f, 0.0f};
                return grad_stage_sums(gs);  // lanes 0..15: candidates 0, 1; lanes 16..31: candidates 2, 3
            }, [&](uint32_t id, uint32_t q, float sum) {
                if (q < kSlots) atomicAdd(rows + (size_t)id * 8u + q, sum);  // no-return global_atomic_add_f32
            });
        }
    };
    __device__ GSRT_INLINE Share share(const uint32_t* ids) const { return Share{{ids, rows}}; }
};

// ---- forward outputs. What a forward kind adds to the blend is one type, its output (V::Out); blend_hit, lane_pass,
// cor_ray and PixelSums name no kind and call it. Sums, zero: the floats it adds to a pixel's sums and, in a forward
// frame, to the ray (CorRay::k), each a sum of x w over the blended hits. blend: a blended hit's share on the blending
// lanes, w its weight, z its view depth, c its place in stage stg (wave-uniform in blend_hit, the lane's own in
// lane_pass). each, each_at: every float in a fixed order, unrolled, alone or with its entry for pixel pix of the
// output's own row-major image (never packed). rows, row_pieces, own_table: the table staged beside the records
// (stage_issue), a row's 16-B pieces, and whether it is the output's own, staged in every frame, or the scene's SH rows.
struct ColourOut {  // colour alone: plain, stats and every gradient kind, whose ray holds its sink's payload in k
    struct Sums {};
    static constexpr uint32_t row_pieces = 12; static constexpr bool own_table = false;
    __device__ GSRT_INLINE static const float* rows() { return kargs().a.sh; }
    template <class K> __device__ GSRT_INLINE static void zero(K&) {}
    template <class K> __device__ GSRT_INLINE static void blend(K&, float, float, const Stage*, uint32_t) {}
    template <class Op> __device__ GSRT_INLINE static void each(Sums&, Op) {}
    template <class Op> __device__ GSRT_INLINE static void each_at(Sums&, size_t, Op) {}
};
// depth (GSRT_FLAG_DEPTH): colour's table, and D, the sum of z w (the expected view depth, premultiplied), to depth_out.
// z is already in a register from the caller's read of the record (a read of its own measured 1.5 % on the depth kernel)
struct DepthOut : ColourOut {
    struct Sums { float D; };
    __device__ GSRT_INLINE static void zero(Sums& s) { s.D = 0.0f; }
    __device__ GSRT_INLINE static void blend(Sums& k, float w, float z, const Stage*, uint32_t) { k.D = fmaf(z, w, k.D); }
    template <class Op> __device__ GSRT_INLINE static void each(Sums& s, Op op) { op(s.D); }
    template <class Op>
    __device__ GSRT_INLINE static void each_at(Sums& s, size_t pix, Op op) { op(s.D, kargs().a.depth_out + pix); }
};
// feat (GSRT_FLAG_FEATURES): F, the sums of f_k w over the candidate's staged row of the feature table (in blend_hit a
// wave-uniform address: four broadcast ds_read_b128); to feat_out, feat_channels floats per pixel (a uniform guard)
struct FeatureOut {
    struct Sums { float F[16]; };
    static constexpr uint32_t row_pieces = 4; static constexpr bool own_table = true;
    __device__ GSRT_INLINE static const float* rows() { return kargs().a.feat_rows; }
    __device__ GSRT_INLINE static void zero(Sums& s) { each(s, [](float& v) { v = 0.0f; }); }  // not Sums{}: DESIGN.md 3
    __device__ GSRT_INLINE static void blend(Sums& k, float w, float, const Stage* stg, uint32_t c) {
        const float4* frow = reinterpret_cast<const float4*>(&stg->sh[0][0][0]) + 4 * c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 f = frow[q];
            k.F[4 * q + 0] = fmaf(f.x, w, k.F[4 * q + 0]);
            k.F[4 * q + 1] = fmaf(f.y, w, k.F[4 * q + 1]);
            k.F[4 * q + 2] = fmaf(f.z, w, k.F[4 * q + 2]);
            k.F[4 * q + 3] = fmaf(f.w, w, k.F[4 * q + 3]);
        }
    }
    template <class Op> __device__ GSRT_INLINE static void each(Sums& s, Op op) {
#pragma unroll
        for (int q = 0; q < 16; ++q) op(s.F[q]);
    }
    template <class Op> __device__ GSRT_INLINE static void each_at(Sums& s, size_t pix, Op op) {
        const uint32_t C = kargs().a.feat_channels;
        float* of = kargs().a.feat_out + pix * C;
#pragma unroll
        for (int q = 0; q < 16; ++q) if ((uint32_t)q < C) op(s.F[q], of + q);
    }
};

// ---- the variants of k_render_cor. A frame is of one kind: plain colour, the counting pass (GSRT_FLAG_STATS), colour
// with the expected view depth (GSRT_FLAG_DEPTH, RenderArgs::depth_out), a feature frame (GSRT_FLAG_FEATURES, feat_out)
// or a gradient frame of the kind RenderSync::grad_kind names (the sinks above). SH: the scene's SH-3 rows are blended;
// LUT: the ExpLUT instead of the exact exponential. Twenty-six kernels: {plain, stats, depth, opgrad} x SH x LUT,
// {feat, grad, shgrad} x LUT and {splatgrad, splatdepthgrad} x SH (never with the LUT, frame_refusal), named by cor_kernel and nowhere
// else. What a forward kind adds sits in its output type, what a gradient kind adds in its sink: the other kinds' code
// does not change, and the shading loop names no kind but stats, another loop body and no output. The RGBA of feat and
// grad is the no-SH frame's. A new forward kind supplies: a CorKind, its output type and line in Out, a line in `waves`,
// a case in cor_kernel, launch_cor. A new gradient kind: a CorKind, its sink and line in Grad, and the same three.
enum class CorKind { plain, stats, depth, feat, grad, shgrad, opgrad, splatgrad, splatdepthgrad };
// waves/SIMD asked for the two feat kernels, from the compiler's register report (109 VGPRs; at 5 and 6 waves they
// spill to scratch)
constexpr uint32_t kFeatWaves = 4;
// and for the two grad kernels, likewise (96 VGPRs, no spill at 5 waves; at 6 the no-LUT kernel spills 12 VGPRs to scratch
// and the LUT kernel stays at 96; 5 measured 4-5 % faster than 4: DESIGN.md section 3); A/B builds: GSRT_GRAD_WAVES
constexpr uint32_t kGradWaves = GSRT_GRAD_WAVES;
// and for the two shgrad kernels, likewise (GSRT_SHGRAD_WAVES)
constexpr uint32_t kShGradWaves = GSRT_SHGRAD_WAVES;
// and for the four opgrad kernels, likewise (GSRT_OPGRAD_WAVES): 127 VGPRs with SH rows and 94 / 95
// without, no scratch at 4; at 5 both SH kernels spill (63 and 66 VGPRs to scratch), at 6 two kernels do
constexpr uint32_t kOpGradWaves = GSRT_OPGRAD_WAVES;
// and for the two splatgrad kernels, likewise (GSRT_SPLATGRAD_WAVES): a stage's 24 terms per lane
// beside opgrad's registers, 155 VGPRs with SH rows and 103 without, no scratch at 3; at 4 the SH kernel spills 24 VGPRs
constexpr uint32_t kSplatGradWaves = GSRT_SPLATGRAD_WAVES;
// and for the two splatdepthgrad kernels, likewise (GSRT_SPLATDEPTHGRAD_WAVES): a stage's 28 terms per
// lane and three more payload floats beside splatgrad's registers, 163 VGPRs with SH rows and 106 without, no scratch at
// 3; at 4 the SH kernel spills 54 VGPRs (84 B of scratch a lane)
constexpr uint32_t kSplatDepthGradWaves = GSRT_SPLATDEPTHGRAD_WAVES;
template <CorKind K, bool SH, bool LUT>
struct CorVariant {
    static constexpr bool sh = SH, lut = LUT;
    static constexpr bool stats = K == CorKind::stats, depth = K == CorKind::depth;
    static constexpr bool feat = K == CorKind::feat, grad = K == CorKind::grad, shgrad = K == CorKind::shgrad;
    static constexpr bool opgrad = K == CorKind::opgrad, splatgrad = K == CorKind::splatgrad;
    static constexpr bool splatdepthgrad = K == CorKind::splatdepthgrad;
    static constexpr bool resweep = opgrad || splatgrad || splatdepthgrad;  // every pass is shaded twice: finals, then the sink's terms
    static constexpr bool grey = feat || grad;  // colour 1: the blend keeps C[0] alone, PixelSums::take replicates it
    static_assert(!(splatgrad || splatdepthgrad) || !LUT, "under the LUT d(alpha) / dg is a segment's slope, not -alpha");
    static_assert(!shgrad || SH, "an SH gradient frame blends the SH rows");
    // waves/SIMD targets (VGPR budget 512 / waves): the three 1-KB stage buffers + ids make 6 KB of LDS per wave, so
    // at most 26 waves per CU; 6 per SIMD (80 VGPRs) for both variants. The no-SH kernel asked for 8 before the
    // third stage buffer, and the compiler, unable to reach it, left it at 101 VGPRs = 4 waves (C4 -6 %, C5 -12 %).
    // The plain SH + LUT kernel asks for the 5 it had at a target of 4 (96 VGPRs) before the SH colours went per lane: left at 4 it takes 102.
    static constexpr uint32_t waves =
        splatdepthgrad ? kSplatDepthGradWaves : splatgrad ? kSplatGradWaves : opgrad ? kOpGradWaves : shgrad ? kShGradWaves : grad ? kGradWaves : feat ? kFeatWaves
        : SH ? (LUT ? (K == CorKind::plain ? 5 : 4) : 6) : (LUT ? 5 : 6);
    // a gradient kind's sink, a forward kind's output, and which of the two holds the ray's own state (CorRay::k)
    using Grad = std::conditional_t<grad, FeatureGrad, std::conditional_t<shgrad, ShGrad, std::conditional_t<
                     opgrad, OpacityGrad, std::conditional_t<splatgrad, SplatGrad, std::conditional_t<
                     splatdepthgrad, SplatDepthGrad, NoGrad>>>>>;
    // a resweep kind's first sweep: the plain blend, which for splatdepthgrad also leaves the ray's D
    using Finals = std::conditional_t<splatdepthgrad, SplatDepthGrad::Finals, NoGrad>;
    using Out = std::conditional_t<depth, DepthOut, std::conditional_t<feat, FeatureOut, ColourOut>>;
    static constexpr bool forward = std::is_same_v<Grad, NoGrad>;
    using RayPayload = std::conditional_t<forward, typename Out::Sums, typename Grad::Payload>;
    // stage geometry (stage_issue): a staged row's 16-B pieces, pieces per stage (4 a record), DMA instructions per stage
    static constexpr uint32_t row_pieces = Out::row_pieces;
    static constexpr uint32_t stage_pieces = (4 + (SH || Out::own_table ? row_pieces : 0)) * kGroup;
    static constexpr uint32_t stage_ops = (stage_pieces + 63) / 64;
    static_assert(!(grad || Out::own_table) || !SH, "no SH in feature gradient frames, nor beside an output's own table");
};
// z: the candidate's view depth (SplatRec::depth), for the frame's output (V::Out). A grey kind's colour (1, as without
// SH) goes into C[0] alone. grad: the stage's share of the frame's sink, told of the hit where some lane blends
template <class V, class Sh>
__device__ GSRT_INLINE uint64_t blend_hit(const Stage* stg, uint32_t c, float z, float alpha, uint64_t contrib,
                                          CorRay<V>& ray, Sh& grad) {
    const float tn = ray.T * (1.0f - alpha);
    const uint64_t low = __ballot(tn < 1e-4f);  // one compare serves both masks
    const uint64_t term = contrib & low;
    const uint64_t blend = contrib & ~low;  // the wave-uniform branch and the mask of the accumulate
    if (blend) {
        float col[3] = {1.0f, 1.0f, 1.0f};
        if (V::sh) ShFromStage{stg, c}(ray.bs, col);
        grad.hit(c, blend, alpha, col, ray);  // T is updated below
        if (lane_of(blend)) {
            const float w = alpha * ray.T;
            ray.C[0] = fmaf(col[0], w, ray.C[0]);
            if constexpr (!V::grey) {
                ray.C[1] = fmaf(col[1], w, ray.C[1]);
                ray.C[2] = fmaf(col[2], w, ray.C[2]);
            }
            V::Out::blend(ray.k, w, z, stg, c);
            grad.hit_lane(c, alpha, col, ray);  // the colour after this hit, ray.T still T_i
            ray.T = tn;
            if (V::stats) ++ray.blended;
        }
    }
    if (term) {  // wave-uniform: a ray stops once
        if (lane_of(term)) {
            ray.active = false;
            ray.pxs = __builtin_nanf("");  // every later g is NaN: the g-first test fails without an active flag
            if (V::stats) ++ray.term;
        }
    }
    return term;
}

// The SH colour kinds (plain and depth frames with SH rows) run phase 2 of a stage per lane. Slab test, exp and alpha
// depend only on the (lane, candidate) pair, and T and the stop are ordered per lane: nothing in phase 2 crosses lanes.
// Pass J so handles every lane's J-th g-passing candidate of the stage end to end (lane_pass), and a stage runs as many
// passes as its busiest lane passes g on candidates, not one per candidate that some lane passes g on.
template <class V>
constexpr bool kShPerLane = V::sh && !V::stats && !V::shgrad && !V::resweep;
// Pass J of a stage. at[J][c] = the lanes whose J-th g-passing candidate is candidate c (c >= J), gone = the lanes whose
// ray stopped in an earlier pass of this stage. The lane selects its candidate index and its g by the masks and reads its
// candidate's record and, where it blends, SH row at its own address: the stage's records lie 64 B = 16 banks apart and
// its rows 192 B = 48 banks, so lanes reading the same 16-B piece of different records or rows meet four distinct 4-bank
// groups and a ds_read_b128 costs its 4 LDS-array cycles as a broadcast read does. Everything up to the masks runs for
// the whole wave, as in shade_stage's phase 2 (the masks are ballots: wave-uniform values, formed outside divergent
// code); a lane outside the pass reads candidate J's record and drops out of every mask.
// The record's layout is per lane here. slab_hit_rel takes min and max of each axis pair, so on an ordered (near, far)
// record it is ray_box_test as on a general one (gsrt_device.hpp, slab_hit_ordered: the same t and u for a ray that can
// reach the box, a miss for any other): when every lane of the pass holds an ordered record the cheap test runs,
// otherwise slab_hit_rel for the pass, with the same result on every lane.
// A lane meets its candidates in ascending c, with blend_hit's tests, weights and colour chain on the same values.
// Returns false when no lane has a J-th candidate left (so none has a later one).
template <class V, uint32_t J>
__device__ GSRT_INLINE bool lane_pass(const Stage* stg, const uint64_t (&at)[kGroup][kGroup], const float (&gv)[kGroup],
                                      uint64_t& gone, const float* lut_s, CorRay<V>& ray) {
    constexpr bool LUT = V::lut;
    uint64_t any = at[J][J];
    if constexpr (J + 1 < kGroup) any |= at[J][J + 1];
    if constexpr (J + 2 < kGroup) any |= at[J][J + 2];
    if constexpr (J + 3 < kGroup) any |= at[J][J + 3];
    any &= ~gone;
    if (!any) return false;  // wave-uniform
    uint32_t cj = J;
    float g = gv[J];
    if constexpr (J + 1 < kGroup) {
        const bool here = lane_of(at[J][J + 1]);
        cj = here ? J + 1 : cj, g = here ? gv[J + 1] : g;
    }
    if constexpr (J + 2 < kGroup) {
        const bool here = lane_of(at[J][J + 2]);
        cj = here ? J + 2 : cj, g = here ? gv[J + 2] : g;
    }
    if constexpr (J + 3 < kGroup) {
        const bool here = lane_of(at[J][J + 3]);
        cj = here ? J + 3 : cj, g = here ? gv[J + 3] : g;
    }
    float4 q0 = reinterpret_cast<const float4*>(&stg->rec[cj])[0];        // lo or near, depth
    const float4 q1 = reinterpret_cast<const float4*>(&stg->rec[cj])[1];  // hi or far, +-opacity
    asm volatile("" : "+v"(q0.w));  // one ds_read_b128, not a ds_read_b96 (shade_stage)
    const float lo[3] = {q0.x, q0.y, q0.z}, hi[3] = {q1.x, q1.y, q1.z};
    const uint64_t general = any & __ballot((int)__float_as_uint(q1.w) < 0);  // the opacity words' sign bits
    const uint64_t ok = any & (general ? __ballot(slab_hit_rel(ray.R, lo, hi)) : __ballot(slab_hit_ordered(ray.R, lo, hi)));
    // the LUT index must stay in range on every lane (g in [0, kGMax]); exp_neg_nocheck takes any g (shade_stage)
    const float gs = LUT ? (lane_of(ok) ? g : 0.0f) : g;
    const float e = LUT ? linear_exp(lut_s, gs) : exp_neg_nocheck(-gs);
    const float alpha = __builtin_fminf(fabsf(q1.w) * e, 0.99f);  // v_min: never NaN where it is kept (shade_stage)
    const uint64_t contrib = ok & __ballot(alpha > kAlphaMin);
    const float tn = ray.T * (1.0f - alpha);
    const uint64_t low = __ballot(tn < 1e-4f);  // one compare serves both masks
    const uint64_t term = contrib & low;
    const uint64_t blend = contrib & ~low;
#ifdef GSRT_DIAG
    ray.dg_lane_max += 1u;
    ray.dg_lanes_g += (uint32_t)__popcll(any);
    ray.dg_lanes_blend += (uint32_t)__popcll(blend);
#endif
    if (blend) {  // wave-uniform: no row read when no lane of the pass blends
        if (lane_of(blend)) {
            float col[3];
            ShFromStage{stg, cj}(ray.bs, col);
            const float w = alpha * ray.T;  // the blend's own weight
            ray.C[0] = fmaf(col[0], w, ray.C[0]);
            ray.C[1] = fmaf(col[1], w, ray.C[1]);
            ray.C[2] = fmaf(col[2], w, ray.C[2]);
            V::Out::blend(ray.k, w, q0.w, stg, cj);
            ray.T = tn;
        }
    }
    if (term) {  // wave-uniform: a ray stops once, and leaves the stage's later passes
        if (lane_of(term)) {
            ray.active = false;
            ray.pxs = __builtin_nanf("");  // see blend_hit
        }
        gone |= term;
    }
    return true;
}
// okg[c]: the lanes that pass g on candidate c (phase 1), gv[c] their g
template <class V>
__device__ GSRT_INLINE void shade_lanes(const Stage* stg, const uint64_t (&okg)[kGroup], const float (&gv)[kGroup],
                                        const float* lut_s, CorRay<V>& ray) {
    static_assert(kGroup == 4, "two bit planes count a lane's earlier candidates; lane_pass selects among four");
    if (!(okg[0] | okg[1] | okg[2] | okg[3])) return;  // wave-uniform: no lane passes g in this stage
#ifdef GSRT_DIAG
    ray.dg_stages_blend += 1u;  // here: stages some lane passes g in
#endif
    // the lanes' counts of earlier g-passing candidates as two bit planes (p1 p0), candidate by candidate
    uint64_t at[kGroup][kGroup];
    uint64_t p0 = 0, p1 = 0;
#pragma unroll
    for (uint32_t c = 0; c < kGroup; ++c) {
        const uint64_t b = okg[c];
        at[0][c] = b & ~p0 & ~p1;
        at[1][c] = b & p0 & ~p1;
        at[2][c] = b & ~p0 & p1;
        at[3][c] = b & p0 & p1;
        const uint64_t carry = p0 & b;
        p0 ^= b;
        p1 ^= carry;
    }
    uint64_t gone = 0;
    if (!lane_pass<V, 0>(stg, at, gv, gone, lut_s, ray)) return;
    if (!lane_pass<V, 1>(stg, at, gv, gone, lut_s, ray)) return;
    if (!lane_pass<V, 2>(stg, at, gv, gone, lut_s, ray)) return;
    lane_pass<V, 3>(stg, at, gv, gone, lut_s, ray);
}

// Shade candidates 0..m of one stage (sorted front to back) for every lane's ray. FULL: m == kGroup is known at
// compile time (the steady state of shade_sorted), so no candidate is tested against m.
// grad: the stage's share of the frame's sink; its terms go to the sink's table once the stage is shaded (flush).
template <class V, bool FULL, class Sh>
__device__ GSRT_INLINE void shade_stage(const Stage* stg, uint32_t m, const float* lut_s, CorRay<V>& ray, Sh grad) {
    constexpr bool LUT = V::lut;
    if constexpr (!V::stats) {
        // Phase 1, g of all kGroup candidates at once (independent chains, one LDS wait): g first because lanes
        // that miss mostly fail it, and a candidate no lane passes is skipped with one wave-uniform branch.
        // g <= gcut = max(0, min(kGMax, ln(255 op) + 0.01)) drops only alphas <= 1/255: the result is
        // unchanged. g in [0, gcut] is one unsigned compare of the bit patterns: gcut >= +0 (k_project); g is
        // never -0 (its first term (A/2 dx) dx is +0 or positive and an exact cancellation rounds to +0); a
        // negative g has the sign bit set; a terminated or invalid ray has pxs = NaN, so g is NaN and fails.
        // okg[c] is the wave's lane mask of candidate c (a ballot: an SGPR pair, no VGPR flag per lane).
        float gv[kGroup];
        uint64_t okg[kGroup];
#pragma unroll
        for (uint32_t c = 0; c < kGroup; ++c) {
            const float4 q2 = reinterpret_cast<const float4*>(&stg->rec[c])[2];  // ppx, ppy, A/2, B
            float4 q3 = reinterpret_cast<const float4*>(&stg->rec[c])[3];        // C/2, gcut, valid, pad
            asm volatile("" : "+v"(q3.w));  // one ds_read_b128 per record (4 LDS-array cycles), not ds_read2_b64 pairs (8)
            const float c2 = q3.x, cut = LUT ? kGMax : q3.y;
            const float dx = ray.pxs - q2.x, dy = ray.pys - q2.y;
            gv[c] = fmaf(c2 * dy, dy, fmaf(q2.w * dx, dy, (q2.z * dx) * dx));
            okg[c] = (FULL || c < m) ? __ballot(__float_as_uint(gv[c]) <= __float_as_uint(cut)) : 0;  // stale records past m: never
        }
#ifdef GSRT_DIAG
        ray.dg_staged += __ballot(ray.active) ? m : 0u;
        ray.dg_stages += __ballot(ray.active) ? 1u : 0u;
        if (__ballot(ray.active)) {
            const uint64_t two = (okg[0] & okg[1]) | (okg[2] & okg[3]) | ((okg[0] | okg[1]) & (okg[2] | okg[3]));
            const uint64_t three = (okg[0] & okg[1] & (okg[2] | okg[3])) | (okg[2] & okg[3] & (okg[0] | okg[1]));
            ray.dg_g_any += (okg[0] ? 1u : 0u) + (okg[1] ? 1u : 0u) + (okg[2] ? 1u : 0u) + (okg[3] ? 1u : 0u);
            ray.dg_g_lane_max += (okg[0] & okg[1] & okg[2] & okg[3]) ? 4u : three ? 3u : two ? 2u
                                 : (okg[0] | okg[1] | okg[2] | okg[3]) ? 1u : 0u;
        }
#endif
        // Phase 2. The SH colour kinds: per lane, in passes (shade_lanes). The others, front to back over the candidates
        // some lane passed: slab test, exp, alpha, blend
        if constexpr (kShPerLane<V>) shade_lanes<V>(stg, okg, gv, lut_s, ray);
        else
#pragma unroll
        for (uint32_t c = 0; c < kGroup; ++c) {
            if (!okg[c]) continue;
            float4 q0 = reinterpret_cast<const float4*>(&stg->rec[c])[0];  // lo or near, depth
            const float4 q1 = reinterpret_cast<const float4*>(&stg->rec[c])[1];  // hi or far, +-opacity
            // q0.w (depth) is unused outside depth frames, but reading all 16 B keeps one ds_read_b128 (4 LDS-array cycles)
            // instead of a ds_read_b96 (8)
            asm volatile("" : "+v"(q0.w));
            // the slab test and exp run for the whole wave; a lane keeps alpha only if it passed both tests. The
            // record's layout (k_project) is wave-uniform: (near, far) when the opacity word is positive
            const float lo[3] = {q0.x, q0.y, q0.z}, hi[3] = {q1.x, q1.y, q1.z};
            const bool ordered = (int)__builtin_amdgcn_readfirstlane(__float_as_uint(q1.w)) >= 0;
            const uint64_t ok = okg[c] & (ordered ? __ballot(slab_hit_ordered(ray.R, lo, hi))
                                                  : __ballot(slab_hit_rel(ray.R, lo, hi)));
            // the LUT index must stay in range on every lane (g in [0, kGMax]); exp_neg_nocheck takes any g (a
            // failed lane's value, even NaN, is discarded below)
            const float gs = LUT ? (lane_of(ok) ? gv[c] : 0.0f) : gv[c];
            const float e = LUT ? linear_exp(lut_s, gs) : exp_neg_nocheck(-gs);
            // min(a, 0.99) as v_min: a is never NaN where it is kept (ok: g in [0, gcut], e in (0, 1])
            const float a = __builtin_fminf(fabsf(q1.w) * e, 0.99f);
            const uint64_t contrib = ok & __ballot(a > kAlphaMin);
            const float alpha = lane_of(contrib) ? a : 0.0f;
#ifdef GSRT_DIAG
            ray.dg_gpass += 1u;
            ray.dg_lanes_g += (uint32_t)__popcll(okg[c]);
            ray.dg_contrib += __ballot(alpha > 0.0f) ? 1u : 0u;
            ray.dg_blend += __ballot(alpha > 0.0f && ray.T * (1.0f - alpha) >= 1e-4f) ? 1u : 0u;
            ray.dg_lanes_blend += (uint32_t)__popcll(__ballot(alpha > 0.0f && ray.T * (1.0f - alpha) >= 1e-4f));
#endif
            grad.candidate(e, fabsf(q1.w), &stg->rec[c]);  // what a hit's term may need besides the blend's own values
            // lanes whose ray stopped here leave the stage's later masks, under one wave-uniform branch
            const uint64_t stopped = blend_hit<V>(stg, c, q0.w, alpha, contrib, ray, grad);
            if (stopped) {
#pragma unroll
                for (uint32_t c1 = c + 1; c1 < kGroup; ++c1) okg[c1] &= ~stopped;
            }
        }
        if (grad.mask) grad.flush();  // wave-uniform: a stage no lane blended adds nothing
    } else {
        for (uint32_t c = 0; c < m; ++c) {
            // counting pass: every AABB candidate of every active ray is counted (no g-first skip)
            const float4* r4 = reinterpret_cast<const float4*>(&stg->rec[c]);
            float4 q0 = r4[0], q1 = r4[1], q2 = r4[2], q3 = r4[3];
            asm volatile("" : "+v"(q1.w), "+v"(q2.x), "+v"(q2.y), "+v"(q2.z), "+v"(q2.w), "+v"(q3.x), "+v"(q3.z));
            float alpha = 0.0f;
            if (ray.active) {
                const float lo[3] = {q0.x, q0.y, q0.z}, hi[3] = {q1.x, q1.y, q1.z};  // relative to the origin
                if (slab_hit_rel(ray.R, lo, hi)) {
                    ++ray.cand;
                    const float dx = ray.pxs - q2.x, dy = ray.pys - q2.y;  // ppx, ppy
                    // A/2 = q2.z, B = q2.w, C/2 = q3.x: = 0.5 fma(C dy, dy, fma(2B dx, dy, (A dx) dx)) exactly
                    const float g = fmaf(q3.x * dy, dy, fmaf(q2.w * dx, dy, (q2.z * dx) * dx));
                    if (g >= 0.0f && g <= kGMax) {
                        const float e = LUT ? linear_exp(lut_s, g) : exp_neg(-g);
                        float a = fabsf(q1.w) * e;  // opacity (negated on a general-layout record, k_project)
                        if (a > 0.99f) a = 0.99f;
                        if (a > kAlphaMin) alpha = a;
                    }
                }
            }
            blend_hit<V>(stg, c, q0.w, alpha, __ballot(alpha > 0.0f), ray, grad);
        }
    }
}


// Shade ids[0..count) (sorted front to back) for every lane's ray; returns false once no lane is active.
// Three stage buffers: while stage k is shaded, the DMAs of stages k+1 and k+2 are in flight; wait_stage waits
// for stage k's own DMA only. No DMA stays in flight past a return (the LDS is reused by the next round or by
// the next workgroup).
// sink: where a gradient frame's terms go (V::Grad, or NoGrad). Every shaded stage then also adds its share to the
// sink's table (shade_stage); its atomics are younger than the DMAs the counted waits wait for, so those waits only
// become stricter, and the last wait covers them too.
template <class V, class S>
__device__ GSRT_INLINE bool shade_sorted(const uint32_t* ids, uint32_t count, Stage* stA, Stage* stB, Stage* stC,
                             const float* lut_s, CorRay<V>& ray, const SplatRec* recs, const float* sh, S sink) {
    const uint32_t lane = lane_id();
    count = __builtin_amdgcn_readfirstlane(count);  // wave-uniform: stage bounds as scalar compares
    if (count == 0) return __ballot(ray.active) != 0;
    auto issue = [&](uint32_t g, Stage* dst) { stage_issue<V>(ids, count, g, lane, dst, recs, sh); };
    auto shade = [&](Stage* stg, uint32_t g) {
        const uint32_t m = count - g < kGroup ? count - g : kGroup;
        shade_stage<V, false>(stg, m, lut_s, ray, sink.share(ids + g));
    };
    auto shade_full = [&](Stage* stg, uint32_t g) {
        shade_stage<V, true>(stg, kGroup, lut_s, ray, sink.share(ids + g));
    };
    constexpr uint32_t kWaitTwo = 2 * V::stage_ops;  // the two younger stages' DMAs stay in flight
    // stages issued after stage g's DMA when it is read: those of g + kGroup and g + 2 kGroup that exist
    auto wait = [count](uint32_t g) {
        wait_stage<V>((g + kGroup < count ? 1u : 0u) + (g + 2 * kGroup < count ? 1u : 0u));
    };
    issue(0, stA);
    if (kGroup < count) issue(kGroup, stB);
    bool live = true;
    uint32_t g0 = 0;
    // Steady state: the stage triples whose three "two stages ahead" issues all exist (g0 + 4 kGroup < count). Every
    // stage shaded here is full and has two younger stages in flight: unconditional issues, a constant wait, no
    // test against the list's end. It leaves the state the general loop below starts from (stage g0 in stA and, issued
    // after it, stage g0 + kGroup in stB), which shades the rest: at most four stages.
    if (!V::stats) {
        for (; g0 + 4 * kGroup < count; g0 += 3 * kGroup) {
            issue(g0 + 2 * kGroup, stC);
            wait_vmcnt<kWaitTwo>();
            shade_full(stA, g0);
            if (!__ballot(ray.active)) { live = false; break; }
            issue(g0 + 3 * kGroup, stA);
            wait_vmcnt<kWaitTwo>();
            shade_full(stB, g0 + kGroup);
            if (!__ballot(ray.active)) { live = false; break; }
            issue(g0 + 4 * kGroup, stB);
            wait_vmcnt<kWaitTwo>();
            shade_full(stC, g0 + 2 * kGroup);
            if (!__ballot(ray.active)) { live = false; break; }
        }
    }
    for (; live && g0 < count; g0 += 3 * kGroup) {
        if (g0 + 2 * kGroup < count) issue(g0 + 2 * kGroup, stC);
        wait(g0);
        shade(stA, g0);
        if (!__ballot(ray.active)) { live = false; break; }
        const uint32_t g1 = g0 + kGroup;
        if (g1 >= count) break;
        if (g1 + 2 * kGroup < count) issue(g1 + 2 * kGroup, stA);
        wait(g1);
        shade(stB, g1);
        if (!__ballot(ray.active)) { live = false; break; }
        const uint32_t g2 = g1 + kGroup;
        if (g2 >= count) break;
        if (g2 + 2 * kGroup < count) issue(g2 + 2 * kGroup, stB);
        wait(g2);
        shade(stC, g2);
        if (!__ballot(ray.active)) { live = false; break; }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // DMAs issued past the last shaded stage
    __syncthreads();
    return live;
}

// Traversal frontier of each super-group (kSG x kSG tile groups): the top of the BVH walked once per
// super-group instead of once per group. Breadth first from the root against the super-group's frustum; a
// node with a leaf child stops (it goes to the frontier as is), the others are replaced by their children that
// meet the frustum, level by level while the frontier fits kFront. Every node a group's rays can reach lies
// below a frontier node (the group's frustum lies inside the super-group's), so groups start from it.
__device__ GSRT_INLINE void frontier_one(const uint32_t g) {
    __shared__ uint32_t cur[2 * kFront], nxt[2 * kFront], fin[2 * kFront];
    const uint32_t lane = lane_id();
    const KArgs& K = kargs();
    if (g >= K.a.sgroups) return;
    uint32_t* out = K.a.frontier + (size_t)g * (kFront + 1);
    const uint32_t gx = g % K.a.sgroups_x, gy = g / K.a.sgroups_x;
    if (K.a.own.active) {  // a super-group spans kSG * fg tile rows: no group of this rank reads a frontier outside
        const uint32_t span = kSG * K.a.fg;
        if ((gy + 1) * span <= K.a.row0 || gy * span >= K.a.row1) return;
    }
    const uint32_t span_x = kSG * K.a.fg * K.a.tw, span_y = kSG * K.a.fg * K.a.th;
    const Frustum F = make_frustum(K.ubo, (float)(gx * span_x) - 0.5f, (float)(gy * span_y) - 0.5f,
                                   (float)((gx + 1) * span_x) + 0.5f, (float)((gy + 1) * span_y) + 0.5f);
    const BvhNode* nodes = K.a.nodes;
    uint32_t ncur = 0, nfin = 0;
    {
        const float rlo[3] = {K.a.root_box[0], K.a.root_box[1], K.a.root_box[2]};
        const float rhi[3] = {K.a.root_box[3], K.a.root_box[4], K.a.root_box[5]};
        if (!box_outside(F, rlo, rhi)) {
            if (lane == 0) cur[0] = K.a.root_ref;
            ncur = 1;
        }
    }
    __syncthreads();
    while (ncur > 0) {
        uint32_t nn = 0, nf = 0;
        for (uint32_t base = 0; base < ncur; base += 64) {
            const uint32_t i = base + lane;
            uint32_t nc = 0, c0 = 0, c1 = 0;
            bool stays = false;
            if (i < ncur) {
                const uint32_t node = cur[i];
                const BvhNode nd = nodes[node];
                if ((nd.l_ref | nd.r_ref) & kLeafBit) {
                    stays = true;
                    c0 = node;
                } else {
                    if (!box_outside(F, nd.l_lo, nd.l_hi)) { c0 = nd.l_ref; ++nc; }
                    if (!box_outside(F, nd.r_lo, nd.r_hi)) { if (nc) c1 = nd.r_ref; else c0 = nd.r_ref; ++nc; }
                }
            }
            const uint64_t bs = __ballot(stays);
            if (stays) fin[nfin + nf + popc_below(bs)] = c0;
            nf += (uint32_t)__popcll(bs);
            const uint64_t b1 = __ballot(nc >= 1), b2 = __ballot(nc >= 2);
            const uint32_t off = popc_below(b1) + popc_below(b2);
            if (nc >= 1) nxt[nn + off] = c0;
            if (nc >= 2) nxt[nn + off + 1] = c1;
            nn += (uint32_t)__popcll(b1) + (uint32_t)__popcll(b2);
        }
        __syncthreads();
        if (nfin + nf + nn > kFront) break;  // the next level does not fit: keep this one
        nfin += nf;
        for (uint32_t i = lane; i < nn; i += 64) cur[i] = nxt[i];
        ncur = nn;
        __syncthreads();
    }
    for (uint32_t i = lane; i < nfin; i += 64) out[1 + i] = fin[i];
    for (uint32_t i = lane; i < ncur; i += 64) out[1 + nfin + i] = cur[i];
    if (lane == 0) out[0] = nfin + ncur;
}

__global__ __launch_bounds__(64) void k_frontier(const KArgs karg) {
    __builtin_amdgcn_s_setprio(kPrepSetprio);
    (void)karg;
    frontier_one(blockIdx.x);
}

// The COR projection's arguments (k_project's, less the camera: the fused kernel takes it from KArgs)
struct ProjArgs {
    uint32_t n;
    const gsrt_gauss_param* params;
    const gsrt_aabb* aabbs;
    SplatRec* recs;
    BvhNode* nodes;
    const uint32_t* gid_slot;
    float4* footprint;
    unsigned long long* counters;
    RankTiles own;
    uint32_t* keyed;
    uint32_t leaf_fp;
    // rank shares: projection block c takes sorted leaves 64 c .. 64 c + 63 (leaf_gid; keyed is then indexed by sorted
    // leaf), whose splats lie close together, so most blocks hold none the band can see
    const uint32_t* leaf_gid;  // nullptr: block c takes gaussian ids 64 c .. 64 c + 63
    const uint32_t* inband;    // rank shares: the slot's in-band bitmap (k_classify), or nullptr
    uint32_t* depth_unsafe;    // the scene's depth-cull guard word (RenderArgs::depth_unsafe)
};
static_assert(sizeof(KArgs) + sizeof(ProjArgs) <= 4096, "kernel argument segment");

// A pipelined COR frame's prep head in one launch: workgroups [0, sgroups) build the super-group frontiers
// (k_frontier), the others project 64 splats each (k_project<COR>). The two are independent, so they share the
// machine as two streams would, but without the cross-stream event between the frontier and the group lists
// (11-14 us per frame in the kernel traces). The frontier's workgroups come first: they are the longer
// latency chains. One-wave workgroups and <= 80 VGPRs, as k_project (they fill slots that retiring render waves free).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6))) void k_prep_cor(const KArgs karg,
                                                                                          const ProjArgs pa) {
    __builtin_amdgcn_s_setprio(kPrepSetprio);
    (void)karg;
    const uint32_t nfb = kargs().a.sgroups;
    if (blockIdx.x < nfb) {
        frontier_one(blockIdx.x);
        return;
    }
    const uint32_t c = blockIdx.x - nfb;
    const uint32_t p = c * 64 + threadIdx.x;  // the bitmap index: gaussian id, or sorted leaf (leaf_gid)
    // the frame's stats words (see k_project)
    if (p < kCounters && p != kErrWord) pa.counters[p] = 0;
    const uint32_t i = pa.leaf_gid ? (p < pa.n ? pa.leaf_gid[p] : pa.n) : p;
    bool k = true;
    if (i < pa.n) {
        const bool prev = pa.keyed ? ((pa.keyed[p >> 5] >> (p & 31u)) & 1u) != 0 : true;
        if (pa.inband && !((pa.inband[i >> 5] >> (i & 31u)) & 1u)) {
            // no tile of the rank's band can see the splat (k_classify ran project_one's own first test, may_own_box):
            // its keys become +inf as project_one's reject path writes them, without its loads, and only when they may
            // still be finite in this slot
            if (prev) {
                if (pa.nodes) put_node_key(pa.nodes, pa.gid_slot, i, 0x7f800000u);
                pa.recs[i].depth = __uint_as_float(0x7f800000u);
            }
            k = false;
        } else {
            k = project_one<GSRT_MODE_COR>(i, pa.n, kargs().ubo, pa.params, pa.aabbs, pa.recs, pa.nodes, pa.gid_slot,
                                           pa.footprint, pa.own, prev, pa.leaf_fp != 0, pa.depth_unsafe);
        }
    }
    if (pa.keyed) {
        const uint64_t m = __ballot(k);
        if ((threadIdx.x & 31u) == 0 && p < pa.n) pa.keyed[p >> 5] = (uint32_t)(m >> (threadIdx.x & 32u));
    }
}

// A rank share's in-band bitmap (1 bit per gaussian id): whether a tile of the band may see the splat, may_own_box of
// its AABB under the frame's camera (project_one's first test, conservative and monotone in the box). The band fit
// (k_fit_chunks<true>) skips the 256-leaf chunks without a set bit, and k_prep_cor rejects the clear splats without
// loading them. One coalesced pass over the AABBs in id order; one-wave workgroups of 4 x 64 splats.
__global__ __launch_bounds__(64) void k_classify(uint32_t n, const gsrt_ubo ubo, const RankTiles own,
                                                 const gsrt_aabb* __restrict__ aabbs, uint32_t* __restrict__ inband) {
    __builtin_amdgcn_s_setprio(kPrepSetprio);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t i = (blockIdx.x * 4 + q) * 64 + threadIdx.x;
        const bool in = i < n && may_own_box(ubo, aabbs[i], own);
        const uint64_t m = __ballot(in);
        if ((threadIdx.x & 31u) == 0 && i < n) inband[i >> 5] = (uint32_t)(m >> (threadIdx.x & 32u));
    }
}

// First traversal round of the COR tiles, one wave per group of FG x FG tiles: one traversal + footprint
// cull + sort for the group (its frustum and footprint rectangle contain those of its tiles), then every
// tile's list is the group's sorted list filtered by the tile's footprint test (order kept), at most kCap
// entries, written to HBM (lists / list_hdr) for k_render_cor. Replaces a traversal and a sort per tile.
// The group list keeps the kGCap nearest; a tile that reaches its end continues after the group's last key.
template <uint32_t FG>
__global__ __launch_bounds__(64) void k_group_list(const KArgs karg) {
    GSRT_WT_START;
    __shared__ uint64_t keys[kGBuf];
    __shared__ uint32_t stack[kGStack];
    __shared__ float4 trect[FG * FG];      // per tile of the group: the samples' rectangle (x0, x1, y0, y1)
    __shared__ uint32_t tslot[FG * FG];    // local (packed) tile index, or kNoGroup when not this rank's
    __builtin_amdgcn_s_setprio(kPrepSetprio);
    (void)karg;
    const uint32_t lane = lane_id();
    const KArgs& K = kargs();
    if (blockIdx.x >= K.a.groups) return;
    const uint32_t g = K.a.group_order ? K.a.group_order[blockIdx.x] : blockIdx.x;
    const uint32_t gx = g % K.a.groups_x, gy = g / K.a.groups_x;
    constexpr uint32_t kT = FG * FG;
    bool mine = false;
    if (lane < kT) {
        const uint32_t tx = gx * FG + lane % FG, ty = gy * FG + lane / FG;
        uint32_t slot = kNoGroup;
        if (tx < K.a.tiles_x && ty >= K.a.row0 && ty < K.a.row1) {  // a tile of this rank's band: its local slot
            slot = band_index(tx, ty, K.a.row0, K.a.row1, K.a.tiles_x);
            mine = true;
        }
        tslot[lane] = slot;
        const float x0 = (float)(tx * K.a.tw), y0 = (float)(ty * K.a.th);
        trect[lane] = make_float4(x0, x0 + (float)K.a.tw, y0, y0 + (float)K.a.th);
    }
    if (!__ballot(mine)) return;
    FrontRegs front;
    if (K.a.frontier) {  // count and entries in one latency; entries past the count are never read from registers
        const uint32_t* fr = K.a.frontier + (size_t)((gy / kSG) * K.a.sgroups_x + gx / kSG) * (kFront + 1);
        front.n = fr[0];
        front.a = fr[1 + lane];
        front.b = 64 + lane < kFront ? fr[65 + lane] : 0u;
    }
    __syncthreads();
#ifdef GSRT_DIAG
    const unsigned long long dg0 = __builtin_amdgcn_s_memtime();
#endif
    const TileRect rect{(float)(gx * FG * K.a.tw) - 0.5f, (float)(gy * FG * K.a.th) - 0.5f,
                        (float)((gx + 1) * FG * K.a.tw) + 0.5f, (float)((gy + 1) * FG * K.a.th) + 0.5f};
    uint32_t restarts = 0;
    // the test knob GSRT_DEBUG_STACK_LIMIT lowers this stack too
    const uint32_t limit = K.a.stack_limit < kStack ? K.a.stack_limit : kGStack;
    const Collected cl = collect_robust<kGCap, kGBuf, KeyCor, kGroupRegSort, true>(rect, 0, false, keys, stack, KeyCor{}, restarts, true,
                                                                    limit, front, true);
    if (cl.restart) {  // the group traversal failed (stack): every tile of the group traverses for itself
        for (uint32_t t = 0; t < kT; ++t) {
            const uint32_t lt = tslot[t];
            if (lt == kNoGroup) continue;
            const float4 r4 = trect[t];
            const TileRect tr{r4.x - kFpInset, r4.z - kFpInset, r4.y + kFpInset, r4.w + kFpInset};  // = tile_rect
            __syncthreads();
            const Collected c1 = collect_robust(tr, 0, false, keys, stack, KeyCor{}, restarts, true, K.a.stack_limit);
            const uint64_t last = c1.count ? keys[c1.count - 1] : 0ull;
            for (uint32_t i = lane; i < c1.count; i += 64) K.a.lists[(size_t)lt * kCap + i] = (uint32_t)keys[i];
            if (lane == 0)
                K.a.list_hdr[lt] = make_uint4(c1.count | (c1.more ? 0x80000000u : 0u), c1.total, (uint32_t)last,
                                              (uint32_t)(last >> 32));
        }
        return;
    }
    // the group list stays in HBM for the tiles' continuation rounds (k_render_cor)
#ifdef GSRT_DIAG
    const unsigned long long dgw = __builtin_amdgcn_s_memtime();
#endif
    {
        uint64_t* gdst = K.a.glist + (size_t)g * kGStride;
        for (uint32_t i = lane; i < cl.count; i += 64) gdst[i] = keys[i];
        if (lane == 0) {
            const uint64_t gl = cl.count ? keys[cl.count - 1] : 0ull;
            K.a.ghdr[g] = make_uint4(cl.count | (cl.more ? 0x80000000u : 0u), 0u, (uint32_t)gl, (uint32_t)(gl >> 32));
        }
    }
    // filter the sorted group list into the tile lists
#ifdef GSRT_DIAG
    const unsigned long long dg1 = __builtin_amdgcn_s_memtime();
#endif
    const float4* fps = K.a.footprint;
    uint32_t cnt = 0;       // lane t < kT: tile t's list length
    bool trunc = false;     // lane t: tile t cut at kCap
    uint32_t last_i = kNoGroup;  // lane t: group-list index of tile t's last kept entry
    uint32_t pos = cl.count;  // lane t: where tile t resumes in the group list (after its last kept entry when cut)
    const uint32_t my_slot = lane < kT ? tslot[lane] : kNoGroup;  // lane t: tile t's packed slot
    uint32_t mine_mask = 0;  // bit t: tile t is this rank's
#pragma unroll
    for (uint32_t t = 0; t < kT; ++t) mine_mask |= (tslot[t] != kNoGroup) ? (1u << t) : 0u;
    mine_mask = __builtin_amdgcn_readfirstlane(mine_mask);
    // software-pipelined: the next chunk's key and footprint (box + ellipse terms) are loaded before this chunk is
    // filtered, so a chunk's loads wait behind the previous chunk's work instead of stalling the wave
    auto fetch = [&](uint32_t i, uint64_t& k, float4& f, float4& a, float4& b) {
        if (i < cl.count) {
            k = keys[i];
            const uint32_t gid = (uint32_t)k;
            const float4* rec = fps + kFpWords * (size_t)gid;
            f = rec[0];
            a = rec[1];
            b = rec[2];
        }
    };
    uint64_t nkey = 0;
    float4 nfp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), ne0 = nfp, ne1 = nfp;
    fetch(lane, nkey, nfp, ne0, ne1);
#ifdef GSRT_DIAG
    unsigned long long dg_test = 0, dg_out = 0;
#endif
    for (uint32_t base = 0; base < cl.count; base += 64) {
#ifdef GSRT_DIAG
        const unsigned long long dgc0 = __builtin_amdgcn_s_memtime();
#endif
        const uint32_t i = base + lane;
        uint32_t m = 0;  // bit t: this candidate's footprint meets tile t
        const uint64_t key = nkey;
        const float4 fp = nfp, e0 = ne0, e1 = ne1;
        if (base + 64 < cl.count) fetch(i + 64, nkey, nfp, ne0, ne1);
        if (i < cl.count) {
            // the tiles whose rectangle the footprint box can meet, then the exact box and ellipse tests on those
            // tiles only. Tile i spans [i, i + 1] in units v = (x - X0) / tw; the box [v0, v1] meets it iff
            // v0 <= i + 1 and v1 >= i, i.e. ceil(v0 - 1) <= i <= floor(v1). floor(v0 - e) and floor(v1 + e),
            // e = 1e-3, bound that range from outside (v's rounding is below 1e-5 for |v| <= 64)
            const float X0 = (float)(gx * FG * K.a.tw), Y0 = (float)(gy * FG * K.a.th);
            const float itw = 1.0f / (float)K.a.tw, ith = 1.0f / (float)K.a.th;
            // (clamped in float first: empty boxes are +-inf, and huge ones must not overflow the conversion)
            auto tidx = [](float v) { return (int)floorf(__builtin_fminf(__builtin_fmaxf(v, -4.0f), 64.0f)); };
            const int tx0 = max(0, tidx((fp.x - X0) * itw - 1e-3f)), tx1 = min((int)FG - 1, tidx((fp.y - X0) * itw + 1e-3f));
            const int ty0 = max(0, tidx((fp.z - Y0) * ith - 1e-3f)), ty1 = min((int)FG - 1, tidx((fp.w - Y0) * ith + 1e-3f));
            uint32_t cand = 0;
            if (tx0 <= tx1 && ty0 <= ty1) {
                const uint32_t row = ((2u << (tx1 - tx0)) - 1u) << tx0;  // bits tx0..tx1
                for (int ty = ty0; ty <= ty1; ++ty) cand |= row << (ty * FG);
            }
            while (cand) {
                const uint32_t t = (uint32_t)__builtin_ctz(cand);
                cand &= cand - 1u;
                const float x0 = X0 + (float)((t % FG) * K.a.tw), y0 = Y0 + (float)((t / FG) * K.a.th);
                const float x1 = x0 + (float)K.a.tw, y1 = y0 + (float)K.a.th;  // = trect[t] (exact integers)
                const bool in = fp.x <= x1 && fp.y >= x0 && fp.z <= y1 && fp.w >= y0 && ell_meets(e0, e1, x0, x1, y0, y1);
                m |= in ? (1u << t) : 0u;
            }
        }
#ifdef GSRT_DIAG
        const unsigned long long dgc1 = __builtin_amdgcn_s_memtime();
        dg_test += dgc1 - dgc0;
#endif
#pragma unroll
        for (uint32_t t = 0; t < kT; ++t) {
            if (!((mine_mask >> t) & 1u)) continue;
            const uint64_t b = __ballot((m >> t) & 1u);
            if (!b) continue;
            const uint32_t lt = __builtin_amdgcn_readlane(my_slot, t);
            const uint32_t c = __builtin_amdgcn_readlane(cnt, t);
            const uint32_t room = kCap - c;
            const uint32_t rank = popc_below(b);
            const bool keep = ((m >> t) & 1u) && rank < room;
            if (keep) K.a.lists[(size_t)lt * kCap + c + rank] = (uint32_t)key;
            const uint32_t n = (uint32_t)__popcll(b);
            const uint32_t took = n < room ? n : room;
            if (took) {
                // lane holding the last kept candidate: the highest set bit of b, or of the kept ones when cut
                const uint64_t kb = n <= room ? b : __ballot(keep);
                const uint32_t hi = 63u - (uint32_t)__builtin_clzll(kb);
                if (lane == t) {
                    last_i = base + hi;
                    if (n > room) pos = base + hi + 1u;
                }
            }
            if (lane == t) {
                if (n > room && !trunc && !took) pos = base;  // cut before this chunk (list already full)
                cnt = c + took;
                trunc = trunc || n > room;
            }
        }
#ifdef GSRT_DIAG
        dg_out += __builtin_amdgcn_s_memtime() - dgc1;
#endif
    }
    const bool gmore = cl.more;
    const uint64_t glast = cl.count ? keys[cl.count - 1] : 0ull;
    const uint64_t last = last_i != kNoGroup ? keys[last_i] : 0ull;  // lane t: tile t's last kept key
    if (lane < kT && my_slot != kNoGroup) {
        // continuation: after the tile's last key when it was cut at kCap, else after the group's last key
        const uint64_t lo = trunc ? last : (gmore ? glast : last);
        K.a.list_hdr[my_slot] = make_uint4(cnt | ((trunc || gmore) ? 0x80000000u : 0u), pos, (uint32_t)lo,
                                               (uint32_t)(lo >> 32));
    }
#ifdef GSRT_DIAG  // [6] group kernel cycles, [7] of which the tile filter, [5] groups whose list overflowed
    if (lane == 0) {
        const unsigned long long dg2 = __builtin_amdgcn_s_memtime();
        atomicAdd(K.a.counters + 6, dg2 - dg0);
        atomicAdd(K.a.counters + 7, dg2 - dg1);
        atomicAdd(K.a.counters + 22, dg_test);  // per-lane tile tests (with the chunk's footprint loads)
        atomicAdd(K.a.counters + 23, dg_out);   // per-tile list output
        atomicAdd(K.a.counters + 24, dg1 - dgw);  // group list to HBM
        if (gmore) atomicAdd(K.a.counters + 5, 1ull);
        atomicMax(K.a.counters + 4, (unsigned long long)cl.count);
        atomicAdd(K.a.counters + 3, (unsigned long long)cl.count);
    }
#endif
    GSRT_WT_END(1, blockIdx.x);
}

// The next segment of an overflowing group list (launched after k_group_list where tiles hold many samples per
// pixel: a 4x4-tile group then spans few pixels and its list often overflows, C5): the next kGCap keys after the first
// segment's last one, once for the group, appended to its list. Its tiles' continuation rounds then read them from
// the group list (k_render_cor) instead of each traversing the BVH after the first segment's end; the candidates
// and their order are the same either way. A separate kernel, so that k_group_list keeps its registers.
template <uint32_t FG>
__global__ __launch_bounds__(64) void k_group_more(const KArgs karg) {
    __shared__ uint64_t keys[kGBuf];
    __shared__ uint32_t stack[kGStack];
    __builtin_amdgcn_s_setprio(kPrepSetprio);
    (void)karg;
    const uint32_t lane = lane_id();
    const KArgs& K = kargs();
    if (blockIdx.x >= K.a.groups) return;
    const uint32_t g = K.a.group_order ? K.a.group_order[blockIdx.x] : blockIdx.x;
    const uint32_t gx = g % K.a.groups_x, gy = g / K.a.groups_x;
    constexpr uint32_t kT = FG * FG;
    bool mine = false;  // (a group without a tile of this rank's band has no list this frame)
    if (lane < kT) {
        const uint32_t tx = gx * FG + lane % FG, ty = gy * FG + lane / FG;
        mine = tx < K.a.tiles_x && ty >= K.a.row0 && ty < K.a.row1;
    }
    if (!__ballot(mine)) return;
    const uint4 gh = K.a.ghdr[g];
    const uint32_t count = gh.x & 0x7fffffffu;
    // (complete; or the group fell back to per-tile traversals; or its list is at its last segment)
    if (!(gh.x >> 31) || count == 0 || count % kGCap != 0 || count >= kGStride) return;
    FrontRegs front;
    if (K.a.frontier) {
        const uint32_t* fr = K.a.frontier + (size_t)((gy / kSG) * K.a.sgroups_x + gx / kSG) * (kFront + 1);
        front.n = fr[0];
        front.a = fr[1 + lane];
        front.b = 64 + lane < kFront ? fr[65 + lane] : 0u;
    }
    const TileRect rect{(float)(gx * FG * K.a.tw) - 0.5f, (float)(gy * FG * K.a.th) - 0.5f,
                        (float)((gx + 1) * FG * K.a.tw) + 0.5f, (float)((gy + 1) * FG * K.a.th) + 0.5f};
    const uint64_t lo = ((uint64_t)gh.w << 32) | gh.z;
    uint32_t restarts = 0;
    const uint32_t limit = K.a.stack_limit < kStack ? K.a.stack_limit : kGStack;
    const Collected cl = collect_robust<kGCap, kGBuf, KeyCor, kGroupRegSort, true>(rect, lo, true, keys, stack,
                                                                                    KeyCor{}, restarts, true, limit,
                                                                                    front, true);
    if (cl.restart) return;  // (the tiles traverse after the first segment, as without this kernel)
    uint64_t* gdst = K.a.glist + (size_t)g * kGStride + count;
    for (uint32_t i = lane; i < cl.count; i += 64) gdst[i] = keys[i];
    if (lane == 0) {
        const uint64_t gl = cl.count ? keys[cl.count - 1] : lo;
        K.a.ghdr[g] = make_uint4((count + cl.count) | (cl.more ? 0x80000000u : 0u), 0u, (uint32_t)gl, (uint32_t)(gl >> 32));
    }
}

// First traversal round of every COR tile as its own kernel: traversal + sort need few registers, so this
// kernel runs at high occupancy and hides the dependent node loads that the shading kernel (occupancy set by
// its SH-3 blend) cannot. The sorted ids go to HBM (1 KiB per tile); k_render_cor picks them up.
__global__ __launch_bounds__(64) void k_collect_cor(const KArgs karg) {
    __shared__ uint64_t keys[2 * kCap];
    __shared__ uint32_t stack[kStack];
    (void)karg;
    const uint32_t lane = lane_id();
    uint32_t lt;
    TileRect rect;
    {
        const KArgs& K = kargs();
        const uint32_t t = blockIdx.x;
        if (t >= K.a.ntiles_local) return;
        lt = xcd_local_tile(t, K.a.ntiles_local);
        uint32_t tx, ty;
        band_tile(lt, K.a.row0, K.a.row1, K.a.tiles_x, tx, ty);
        rect = tile_rect(tx, ty, K.a.tw, K.a.th);
    }
    const KArgs& K = kargs();
    uint32_t* dst = K.a.lists + (size_t)lt * kCap;
    // without group lists (counting pass, a single Gaussian, GSRT_DEBUG_NO_GROUPS): traverse for this tile
    uint32_t restarts = 0;
    const Collected cl = collect_robust(rect, 0, false, keys, stack, KeyCor{}, restarts, K.a.cull2d != 0);
    const uint64_t last = cl.count ? keys[cl.count - 1] : 0ull;  // continuation key of the next round
    for (uint32_t i = lane; i < cl.count; i += 64) dst[i] = (uint32_t)keys[i];
    if (lane == 0)
        K.a.list_hdr[lt] = make_uint4(cl.count | (cl.more ? 0x80000000u : 0u), cl.total, (uint32_t)last, (uint32_t)(last >> 32));
}

// The tile of a k_render_cor workgroup: wave-uniform values. tw, th and S are powers of two (make_plan): shifts instead
// of divisions. The lane's pixel, its validity and the tile's rectangle are recomputed where they are used (ray setup,
// rare continuation rounds, the store) from these and a laundered lane id, so that none of them lives (spilled) across
// the shading loop.
struct CorTile {
    uint32_t lt;  // packed slot of the tile
    uint32_t x0, y0, tw, th, S, lgS, lgtw, lgth;
    struct Pixel { uint32_t in_tile, s, x, y; bool valid; };  // the lane's pixel, its sample within the pass, inside the frame
    __device__ GSRT_INLINE Pixel pixel() const {
        uint32_t l = lane_id();
        asm volatile("" : "+v"(l));  // a fresh lane id: no live range across the shading loop
        Pixel p;
        p.in_tile = l >> lgS;
        p.s = l & (S - 1u);
        p.x = x0 + (p.in_tile & (tw - 1u));
        p.y = y0 + (p.in_tile >> lgtw);
        p.valid = p.x < kargs().a.width && p.y < kargs().a.height;
        return p;
    }
    __device__ GSRT_INLINE TileRect rect_here() const {
        uint32_t tx = x0 >> lgtw, ty = y0 >> lgth;
        asm volatile("" : "+s"(tx), "+s"(ty));  // recomputed at the (rare) use, not hoisted and spilled
        return tile_rect(tx, ty, tw, th);
    }
};

// What a pixel outputs, summed over its samples: the colour, then what the frame's output adds; each: in that fixed order
template <class V>
struct PixelSums {
    float rgba[4];
    typename V::Out::Sums k;
    template <class Op>
    __device__ GSRT_INLINE void each(Op op) {
#pragma unroll
        for (int q = 0; q < 4; ++q) op(rgba[q]);
        V::Out::each(k, op);
    }
    template <class Op>  // the floats beyond the colour with their entries in the output's own image
    __device__ GSRT_INLINE void each_extra_at(size_t pix, Op op) { V::Out::each_at(k, pix, op); }
    // every float with its entry in its own image; colour: the pixel's four floats
    template <class Op>
    __device__ GSRT_INLINE void each_at(float* colour, size_t pix, Op op) {
#pragma unroll
        for (int q = 0; q < 4; ++q) op(rgba[q], colour + q);
        each_extra_at(pix, op);
    }
    // a finished pass's results (= 0 + x exactly, x >= +0). A grey kind's blend kept one channel (blend_hit)
    __device__ GSRT_INLINE void take(const CorRay<V>& ray) {
        rgba[0] = ray.C[0]; rgba[1] = ray.C[V::grey ? 0 : 1]; rgba[2] = ray.C[V::grey ? 0 : 2]; rgba[3] = 1.0f - ray.T;
        if constexpr (V::forward) k = ray.k;
    }
};

// The ray of the lane's pixel p and sample for one pass, nothing blended yet
template <class V>
__device__ GSRT_INLINE CorRay<V> cor_ray(const CorTile::Pixel& p, uint32_t S, uint32_t pass, uint32_t passes) {
    CorRay<V> ray;
    {
        const KArgs& K = kargs();
        // sample sidx takes draws 2*sidx, 2*sidx+1 of the pixel LCG seeded with Camera.RandomSeed
        // (RayTracing.rgen:27,39: the same sequence for every pixel)
        const uint32_t sidx = pass * S + p.s;
        uint32_t seed = K.ubo.random_seed;
        for (uint32_t q = 0; q < sidx; ++q) { random_float(&seed); random_float(&seed); }
        const float jx = random_float(&seed);
        const float jy = random_float(&seed);
        ray.pxs = (float)p.x + jx;
        ray.pys = (float)p.y + jy;
        float o[3], d[3];
        gen_ray(K.ubo, ray.pxs, ray.pys, o, d);
        ray.R = make_obj_ray(d);
        if (V::sh) sh_basis(d, ray.bs);
    }
    ray.T = 1.0f;
    ray.C[0] = ray.C[1] = ray.C[2] = 0.0f;
    V::Out::zero(ray.k);
    V::Grad::load(ray.k, p.x, p.y, p.valid, S * passes);  // a gradient kind: the pixel's upstream gradient
    ray.active = p.valid;
    if (!p.valid) ray.pxs = __builtin_nanf("");  // see blend_hit
    ray.cand = ray.blended = ray.term = 0;
#ifdef GSRT_DIAG
    ray.dg_staged = ray.dg_gpass = ray.dg_contrib = ray.dg_blend = ray.dg_lanes_g = ray.dg_lanes_blend = 0;
    ray.dg_stages = ray.dg_stages_blend = ray.dg_lane_max = 0;
    ray.dg_g_any = ray.dg_g_lane_max = 0;
#endif
    return ray;
}

// ---- the three sources of a round's candidates. Each leaves the round's ids, sorted front to back, in ids[0..count),
// lo at the last key considered (the next round continues after it) and gpos where the tile resumes in its group's list.
// The first round: the list k_group_list / k_collect_cor wrote, its header and first 128 ids already on their way into
// LDS (list_issue) when prefetched
__device__ GSRT_INLINE Collected round_from_list(const CorTile& t, bool& prefetched, uint32_t* ids, const uint32_t* lhdr,
                                                 uint64_t& lo, uint32_t& gpos) {
    Collected cl{};
    if (!prefetched) list_issue(t.lt, lane_here(), ids, const_cast<uint32_t*>(lhdr));  // later passes: ids[] was reused
    prefetched = false;
    __syncthreads();  // vmcnt(0): header and ids[0..128) landed
    const uint4 h = make_uint4(lhdr[0], lhdr[1], lhdr[2], lhdr[3]);
    const uint32_t* src = kargs().a.lists + (size_t)t.lt * kCap;
    cl.count = h.x & 0x7fffffffu;
    cl.more = (h.x >> 31) != 0;
    for (uint32_t i = 128u + lane_here(); i < cl.count; i += 64) ids[i] = src[i];
    cl.total = cl.count;
    lo = ((uint64_t)h.w << 32) | h.z;
    gpos = h.y;
    __syncthreads();
    return cl;
}
// Continuation inside the group list: the next entries after gpos that meet this tile's footprint test, in order;
// lo = the last entry considered. found: the list had entries left (else the tile traverses for itself)
__device__ GSRT_INLINE Collected round_from_group(const CorTile& t, uint32_t* ids, uint64_t& lo, uint32_t& gpos, bool& found) {
    Collected cl{};
    const KArgs& K = kargs();
    const uint32_t g = (t.y0 / t.th / K.a.fg) * K.a.groups_x + (t.x0 / t.tw / K.a.fg);
    const uint4 gh = K.a.ghdr[g];
    const uint32_t gcount = gh.x & 0x7fffffffu;
    found = gpos < gcount;
    if (!found) return cl;
    const uint64_t* gl = K.a.glist + (size_t)g * kGStride;
    const float4* fps = K.a.footprint;
    const TileRect rect_c = t.rect_here();
    uint32_t out = 0;
    while (gpos < gcount && out < kCap) {
        const uint32_t i = gpos + lane_here();
        bool keep = false;
        uint64_t key = 0;
        if (i < gcount) {
            key = gl[i];
            keep = fp_meets(fps, (uint32_t)key, rect_c);
        }
        const uint64_t b = __ballot(keep);
        const uint32_t rank = popc_below(b), n = (uint32_t)__popcll(b), room = kCap - out;
        if (keep && rank < room) ids[out + rank] = (uint32_t)key;
        if (n > room) {  // cut: resume after the last entry taken
            const uint64_t kb = __ballot(keep && rank < room);
            gpos += (uint32_t)(63 - __builtin_clzll(kb)) + 1u;
            out = kCap;
        } else {
            gpos = gpos + 64u < gcount ? gpos + 64u : gcount;
            out += n;
        }
    }
    cl.count = cl.total = out;
    cl.more = gpos < gcount || (gh.x >> 31) != 0;
    lo = gl[gpos - 1];  // every group entry up to here was considered for this tile
    __syncthreads();
    return cl;
}
// The tile's own traversal for the keys after lo (no group list, or past the end of an overflowing one), the sorted
// keys narrowed to ids
template <class V>
__device__ GSRT_INLINE Collected round_from_traversal(const CorTile& t, uint64_t* keys, uint32_t* stack, uint32_t* ids,
                                                      uint64_t& lo, bool has_lo, uint32_t& restarts) {
    const uint32_t lim = kargs().a.stack_limit < kRStack ? kargs().a.stack_limit : kRStack;
    const Collected cl = collect_robust<kRCap, kRBuf>(t.rect_here(), lo, has_lo, keys, stack, KeyCorRec{}, restarts,
                                                      !V::stats && kargs().a.cull2d, lim, FrontRegs{}, !V::stats);
    lo = cl.count ? keys[cl.count - 1] : lo;
    // narrow the sorted keys to ids in place (ids[i] overlays keys[i/2]: already read, in order)
    const uint32_t ln = lane_here();
    for (uint32_t base = 0; base < cl.count; base += 64) {
        const uint32_t i = base + ln;
        const uint32_t v = i < cl.count ? (uint32_t)keys[i] : 0u;
        asm volatile("" ::: "memory");
        if (i < cl.count) ids[i] = v;
        asm volatile("" ::: "memory");
    }
    __syncthreads();
    return cl;
}

template <class V>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(V::waves)))
void k_render_cor(const KArgs karg) {
    // traversal buffers (keys, stack) and shading buffers (ids, two stages) are never live at once
    union CorLds {
        struct { uint64_t keys[kRBuf]; uint32_t stack[kRStack]; } t;
        struct { uint32_t ids[kCap]; uint32_t hdr[4]; } l;  // hdr: the first round's list header (LDS-DMA)
    };
    __shared__ CorLds L;
    __shared__ Stage stA, stB, stC;
    __shared__ float lut_s[V::lut ? 512 : 1];
    uint64_t* const keys = L.t.keys;
    uint32_t* const stack = L.t.stack;
    uint32_t* const ids = L.l.ids;
    uint32_t* const lhdr = L.l.hdr;
    const SplatRec* const recs = kargs().a.recs;  // stage DMA sources, read once (kargs() is not hoisted)
    const float* const shp = V::Out::rows();
    (void)karg;  // read through kargs()
    const uint32_t lane = lane_id();
#ifdef GSRT_DIAG
    const unsigned long long diag_entry = __builtin_amdgcn_s_memtime();
    unsigned long long diag_setup = 0, diag_last = 0;
#endif
    if (V::lut) {
        const float* lut = kargs().a.lut;
        for (uint32_t i = lane; i < 512; i += 64) lut_s[i] = lut[i];
        __syncthreads();
    }
    GSRT_WT_START;
    // the tile's cost in the partition's profile (RenderArgs::tile_cost): its wave's wall time in ticks of the 100-MHz
    // real-time counter, from here to the store. Counted work (staged and shaded candidates) left the centre bands of
    // an 8-rank C3 frame 28 % slower than the outer ones at equal counts: time also follows the continuation rounds'
    // traversals, the blending depth and the L2 hit rate of the region
    const uint32_t t_tile0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
    // ---- tile setup
    CorTile tile;
    uint32_t passes;
    {
        const KArgs& K = kargs();
        const uint32_t t = blockIdx.x;
        if (t >= K.a.ntiles_local) return;
        tile.lt = xcd_local_tile_perm(t, K.a.ntiles_local, K.a.run_order);
        uint32_t tx, ty;
        band_tile(tile.lt, K.a.row0, K.a.row1, K.a.tiles_x, tx, ty);
        tile.tw = K.a.tw; tile.th = K.a.th; tile.S = K.a.s_lanes; passes = K.a.passes;
        tile.x0 = tx * tile.tw; tile.y0 = ty * tile.th;
    }
    // the first round's list (k_group_list / k_collect_cor wrote it): its header and first 128 ids go straight
    // into LDS (LDS-DMA: no VGPRs held across the setup), issued here so that their latency hides behind the
    // ray setup (the tile's list slot holds kCap entries, so the loads stay inside it whatever the count)
    tile.lt = __builtin_amdgcn_readfirstlane(tile.lt);
    bool prefetched = false;
    if (kargs().a.prelisted) {
        list_issue(tile.lt, lane, ids, lhdr);
        prefetched = true;
    }
    tile.x0 = __builtin_amdgcn_readfirstlane(tile.x0);
    tile.y0 = __builtin_amdgcn_readfirstlane(tile.y0);
    tile.lgS = (uint32_t)__builtin_ctz(tile.S);
    tile.lgtw = (uint32_t)__builtin_ctz(tile.tw); tile.lgth = (uint32_t)__builtin_ctz(tile.th);
    const uint32_t S = tile.S;
    // the pixel's sums over its samples: with one pass (spp <= 64) the pass's own values; with several passes
    // (spp > 64: one pixel per lane) the pixel's entries in the output images hold the running sums between passes, so
    // that no accumulator lives (spilled) across the shading loop. The sums are formed in the same order either way.
    PixelSums<V> sums{};
    uint32_t st_cand = 0, st_blend = 0, st_term = 0, st_rounds = 0, restarts = 0, maxc = 0;
#ifdef GSRT_DIAG  // diagnostic build only: per-wave cycle split between traversal+sort and shading
    unsigned long long diag_collect = 0, diag_shade = 0;
#endif
    for (uint32_t pass = 0; pass < passes; ++pass) {
        CorRay<V> ray = cor_ray<V>(tile.pixel(), S, pass, passes);
        // opgrad, splatgrad and splatdepthgrad (V::resweep): two sweeps over the same rounds. The first is the plain blend and gives the pass its results and the
        // ray its finals; the second sets the ray up again, restarts the rounds from the tile's first list
        // (round_from_list issues it again: prefetched is false by then) and blends the same hits in the same order with
        // the same arithmetic, so that every test falls as it fell, now with the gradient terms (blend_hit)
        // (a do-while whose condition is constant false for every other kind: their loop nest is what it was)
        [[maybe_unused]] uint32_t sweep = 0;
        do {
            uint64_t lo = 0;
            bool has_lo = false;
            uint32_t gpos = 0;  // with group lists: where this tile resumes in its group's sorted list
            for (;;) {
#ifdef GSRT_DIAG
                const unsigned long long d0 = __builtin_amdgcn_s_memtime();
                if (!has_lo) diag_setup += d0 - (pass == 0 ? diag_entry : diag_last);
#endif
                Collected cl;
                bool listed = true;
                if (kargs().a.prelisted && !has_lo) {
                    cl = round_from_list(tile, prefetched, ids, lhdr, lo, gpos);
                } else {
                    listed = false;
                    if (kargs().a.use_groups) cl = round_from_group(tile, ids, lo, gpos, listed);
                }
                if (!listed) cl = round_from_traversal<V>(tile, keys, stack, ids, lo, has_lo, restarts);
#ifdef GSRT_DIAG
                const unsigned long long d1 = __builtin_amdgcn_s_memtime();
                diag_collect += d1 - d0;
#endif
                ++st_rounds;
                if (cl.total > maxc) maxc = cl.total;
                // a gradient kind's terms go to its sink, in a resweep kind's second sweep: the first is the plain blend
                const bool live = V::resweep && sweep == 0
                    ? shade_sorted<V>(ids, cl.count, &stA, &stB, &stC, lut_s, ray, recs, shp, typename V::Finals{})
                    : shade_sorted<V>(ids, cl.count, &stA, &stB, &stC, lut_s, ray, recs, shp, V::Grad::of_frame());
#ifdef GSRT_DIAG
                diag_last = __builtin_amdgcn_s_memtime();
                diag_shade += diag_last - d1;
#endif
                if (!cl.more || !live) break;
                has_lo = true;  // lo = the last (largest) key of this round
                __syncthreads();
            }
            if constexpr (V::resweep) {
                if (sweep == 0) {
                    sums.take(ray);  // once per pass, from the first sweep's values
                    const float fin[4] = {ray.C[0], ray.C[1], ray.C[2], ray.T};
                    [[maybe_unused]] float finD = 0.0f;
                    if constexpr (V::splatdepthgrad) finD = ray.k.D;
                    ray = cor_ray<V>(tile.pixel(), S, pass, passes);
#pragma unroll
                    for (int q = 0; q < 4; ++q) ray.k.fin[q] = fin[q];
                    if constexpr (V::splatdepthgrad) ray.k.finD = finD;
                }
            }
        } while (V::resweep && ++sweep < 2);
        if constexpr (!V::resweep) sums.take(ray);
        if (passes > 1) {  // then S == 1 (make_plan): the lane's pixel accumulates its passes in order, prev + pass
            const CorTile::Pixel p = tile.pixel();
            if (p.valid) {
                const KArgs& K = kargs();
                const size_t pix = (size_t)p.y * K.a.width + p.x;
                float4* o = (K.a.dump8 ? K.a.accum : reinterpret_cast<float4*>(K.a.out)) +
                            (K.a.packed ? (size_t)tile.lt * (tile.tw * tile.th) + p.in_tile : pix);
                if (pass > 0) sums.each_at(&o->x, pix, [](float& v, const float* home) { v = *home + v; });
                if (pass + 1 < passes) sums.each_at(&o->x, pix, [](float v, float* home) { *home = v; });
            }
        }
        st_cand += ray.cand; st_blend += ray.blended; st_term += ray.term;
#ifdef GSRT_DIAG
        if (!V::stats && lane == 0) {
            const uint32_t dg[6] = {ray.dg_staged, ray.dg_gpass, ray.dg_contrib, ray.dg_blend, ray.dg_lanes_g, ray.dg_lanes_blend};
            for (int q = 0; q < 6; ++q) atomicAdd(kargs().a.counters + 16 + q, (unsigned long long)dg[q]);
            const uint32_t ds[3] = {ray.dg_stages, ray.dg_stages_blend, ray.dg_lane_max};
            for (int q = 0; q < 3; ++q) atomicAdd(kargs().a.counters + 25 + q, (unsigned long long)ds[q]);
            atomicAdd(kargs().a.counters + 30, (unsigned long long)ray.dg_g_any);
            atomicAdd(kargs().a.counters + 31, (unsigned long long)ray.dg_g_lane_max);
        }
#endif
    }
    // pairwise reduction over the S in-wave samples of a pixel (the oracle sums in the same tree); partners 1 and
    // 2 lanes away by DPP quad permutes (no LDS round trip), farther ones by shuffles
    if (S > 1) sums.each([](float& v) { v = v + dpp_from<0xB1>(v); });
    if (S > 2) sums.each([](float& v) { v = v + dpp_from<0x4E>(v); });
    for (uint32_t off = 4; off < S; off <<= 1) sums.each([off](float& v) { v = v + __shfl_xor(v, (int)off); });
    for (uint32_t off = 1; V::stats && off < S; off <<= 1) {
        st_cand += __shfl_xor(st_cand, (int)off);
        st_blend += __shfl_xor(st_blend, (int)off);
        st_term += __shfl_xor(st_term, (int)off);
    }
    const KArgs& K = kargs();
    const uint32_t ns = S * passes;
    const CorTile::Pixel p = tile.pixel();
    if (p.valid && p.s == 0) {
        sums.each([ns](float& v) { v = over_samples(v, ns); });
        const float4 v = make_float4(sums.rgba[0], sums.rgba[1], sums.rgba[2], sums.rgba[3]);
        const size_t pix = (size_t)p.y * K.a.width + p.x;
        const size_t idx = K.a.packed ? (size_t)tile.lt * (tile.tw * tile.th) + p.in_tile : pix;
        if (K.a.dump8) {  // the integers the frame dump prints (Dump8), exact values of the rest in the escape list
            const uint32_t code = dump8_code(v);
            reinterpret_cast<uint32_t*>(K.a.out)[idx] = code;
            if (code & kDump8Escape) {
                const uint32_t e = atomicAdd(&K.a.esc[0].x, 1u);
                if (e < K.a.esc_cap)
                    K.a.esc[1 + e] = make_uint4((uint32_t)idx, __float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z));
            }
        } else {
            reinterpret_cast<float4*>(K.a.out)[idx] = v;
        }
        sums.each_extra_at(pix, [](float x, float* home) { *home = x; });
        if (V::stats && K.a.ray_stats)
            reinterpret_cast<uint4*>(K.a.ray_stats)[pix] = make_uint4(st_cand, st_blend, st_rounds, st_term);
    }
#ifdef GSRT_DIAG
    if (lane == 0) {
        atomicAdd(K.a.counters + 9, diag_collect);
        atomicAdd(K.a.counters + 10, diag_shade);
        const unsigned long long dend = __builtin_amdgcn_s_memtime();
        atomicAdd(K.a.counters + 11, dend - diag_entry);
        atomicAdd(K.a.counters + 1, diag_setup);      // entry (or a pass's end) to the first round: tile + ray setup
        atomicAdd(K.a.counters + 2, dend - diag_last);  // last round's end to the end: reduction + store
    }
#endif
    // the partition's cost profile: one store per tile (device-scope atomics on a few row words serialise at the
    // memory side and slowed the frame by several percent)
    if (K.a.tile_cost && lane == 0) K.a.tile_cost[tile.lt] = (uint32_t)__builtin_amdgcn_s_memrealtime() - t_tile0;
    if (V::stats) {
        const uint32_t lead = (p.valid && p.s == 0) ? 1u : 0u;
        add_counters(wave_sum(p.valid ? 1u : 0u) * passes, wave_sum(lead ? st_cand : 0u), wave_sum(lead ? st_blend : 0u),
                     wave_sum(lead ? st_term : 0u), st_rounds, restarts, maxc);
    }
    GSRT_WT_END(0, tile.lt);
}

// ----------------------------------------------------------------------------------------- REF

template <bool STATS>
__global__ __launch_bounds__(64) void k_render_ref(const KArgs karg) {
    __shared__ uint64_t keys[2 * kCap];
    __shared__ uint32_t stack[kStack];
    __shared__ float lut_s[512];
    (void)karg;
    const uint32_t lane = lane_id();
    {
        const float* lut = kargs().a.lut;
        for (uint32_t i = lane; i < 512; i += 64) lut_s[i] = lut[i];
    }
    __syncthreads();
    uint32_t lt, x0, y0, samples, bounces;
    {
        const KArgs& K = kargs();
        const uint32_t t = blockIdx.x;
        if (t >= K.a.ntiles_local) return;
        lt = xcd_local_tile(t, K.a.ntiles_local);
        uint32_t tx, ty;
        band_tile(lt, K.a.row0, K.a.row1, K.a.tiles_x, tx, ty);
        x0 = tx * 8; y0 = ty * 8;
        samples = K.a.samples; bounces = K.a.bounces;
    }
    const uint32_t px = x0 + (lane & 7u), py = y0 + (lane >> 3);
    bool valid;
    float o[3];
    ObjRay R;
    float tri = kTMax;  // min_thit after the triangles (vulkan_ray_tracing.cc:534, 929-931): kTMax = no triangle hit
    {
        const KArgs& K = kargs();
        valid = px < K.a.width && py < K.a.height;
        float d[3];
        gen_ray(K.ubo, (float)px, (float)py, o, d);  // rgen:39-43 at the integer launch id
        R = make_obj_ray(d);
        if (K.a.tri_t && valid) tri = K.a.tri_t[(size_t)py * K.a.width + px];
    }
    const bool tri_hit = tri < kTMax;  // traversal_data.hit_geometry after traceRay (:1094-1096)
    // BLAS boxes entered at or beyond min_thit are culled (:806-807: thit >= min_thit * worldToObject_tMultiplier);
    // with no triangle hit min_thit = Tmax, so only an entry at exactly tmax is dropped
    const float tcut = tri * R.norm;
    const TileRect rect{(float)x0 - 0.5f, (float)y0 - 0.5f, (float)(x0 + 7) + 0.5f, (float)(y0 + 7) + 0.5f};
    uint32_t restarts = 0, st_cand = 0, st_rounds = 0;
    const Collected first = collect_robust(rect, 0, false, keys, stack, KeyRef{}, restarts);
    const bool cached = first.total <= kCap;
    // per-ray state: RayInfo + payload Trans + NextK (Scene.cpp:38-45)
    float Depth = 0.0f, Trans = 1.0f;
    float kd[8], ka[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { kd[j] = kKEmpty; ka[j] = -1.0f; }
    int gnum = 0;
    for (uint32_t s = 0; s < samples; ++s) {
        bool alive = valid;
        for (uint32_t b = 0; b <= bounces; ++b) {
            if (!__ballot(alive)) break;
            // report_ray_intersection_impl (instructions.cc:7036-7050): after a triangle hit, a Gaussian report is
            // accepted only below world_min_thit = the triangle's t
            bool reported = tri_hit, gauss_rep = false;
            float closest = tri;
            if (alive) {
                ++st_rounds;
                gnum = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) kd[j] = kKEmpty;
            }
            uint64_t lo = 0;
            bool has_lo = false;
            for (;;) {  // chunks of kCap candidates in id order (one chunk unless the tile overflowed)
                Collected cl = first;
                if (!cached) cl = collect_robust(rect, lo, has_lo, keys, stack, KeyRef{}, restarts);
                const SplatRec* recs = kargs().a.recs;
                for (uint32_t c = 0; c < cl.count; ++c) {
                    const uint32_t gid = uni((uint32_t)keys[c]);
                    const SplatRec* __restrict__ r = recs + gid;
                    if (!alive) continue;
                    const float rlo[3] = {r->lo[0], r->lo[1], r->lo[2]};
                    const float rhi[3] = {r->hi[0], r->hi[1], r->hi[2]};
                    if (!slab_hit_rel_cut(R, rlo, rhi, tcut)) continue;
                    if (st_rounds == 1) ++st_cand;
                    const float depth = r->depth;
                    if (depth <= Depth) continue;  // rint:69-71
                    const float dx = (float)px - r->ppx, dy = (float)py - r->ppy;
                    const float g = 0.5f * (((r->a * dx) * dx + ((2.0f * r->b) * dx) * dy) + (r->c * dy) * dy);
                    if (g < 0.0f || g > kGMax) continue;  // rint:102
                    if (g != g) continue;                 // NaN never passes alpha > 1/255
                    const float alpha = r->opacity * linear_exp(lut_s, g);
                    if (alpha > kAlphaMin) {
                        float nd = depth, na = alpha;  // InsertNewSplat, rint:35-43
                        bool ins = false;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            if (kd[j] > nd) {
                                const float td = kd[j], ta = ka[j];
                                kd[j] = nd; ka[j] = na;
                                nd = td; na = ta;
                                ins = true;
                            }
                        }
                        if (ins) gnum += 1;
                        // report_ray_intersection_impl (instructions.cc:7040-7046)
                        if (0.001f <= depth && (reported ? depth < closest : depth <= kTMax)) {
                            reported = gauss_rep = true;
                            closest = depth;
                        }
                    }
                }
                if (cached || cl.total <= kCap) break;
                lo = keys[kCap - 1];
                has_lo = true;
                __syncthreads();
            }
            if (alive) {
                if (gauss_rep) {  // rchit:15-33, GaussNum clamped to 8
                    const int m = gnum < 8 ? gnum : 8;
                    float ct = Trans;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (j < m) ct *= (1.0f - ka[j]);
                    Trans = ct;
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (j == m - 1) Depth = kd[j];
                } else if (tri_hit) {
                    Trans = 0.0f;  // the triangle's closest hit: RayTracing.rchit, Scatter() returns RayPayload(0, ...)
                }
                if (gnum == 0) alive = false;  // rgen:64-68
            }
        }
    }
    const KArgs& K = kargs();
    if (valid) {
        const size_t pix = (size_t)py * K.a.width + px;
        reinterpret_cast<float4*>(K.a.out)[K.a.packed ? (size_t)lt * 64 + lane : pix] =
            make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // rgen:33,75: pixelColor is never written
        if (K.a.rs) {
            gsrt_raystate st;
            st.trans = Trans;
            st.depth = Depth;
            st.gauss_num = gnum < 8 ? gnum : 8;
            st.gauss_num_raw = gnum;
#pragma unroll
            for (int j = 0; j < 8; ++j) { st.k[j][0] = kd[j]; st.k[j][1] = ka[j]; }
            K.a.rs[pix] = st;
        }
        if (STATS && K.a.ray_stats) reinterpret_cast<uint4*>(K.a.ray_stats)[pix] = make_uint4(st_cand, 0u, st_rounds, 0u);
    }
    if (STATS) add_counters(wave_sum(valid ? 1u : 0u) * samples, wave_sum(valid ? st_cand : 0u), 0ull, 0ull,
                            uni(st_rounds), restarts, first.total);
}

// VS-style traversal statistics of a REF frame (GSRT_FLAG_STATS; gsrt_vs_stats, vulkan-sim gpu-sim.cc:1510-1518):
// after k_render_ref, one lane per pixel walks the LBVH depth first as VulkanRayTracing::traceRay walks its BVH
// (vulkan_ray_tracing.cc:560-1010: every visited internal node and every reached leaf counts, a child is entered
// when the object ray's slab test passes it and, past a triangle hit, its entry lies below min_thit). The node
// count is the LBVH's, not Embree's: comparable in kind, not in value. Per ray: ray_stats.w = nodes of one
// traversal, ray_stats.y = traversals that hit a triangle (rt_num_hits; every round re-traverses, rgen:58-62);
// counters [24] nodes summed over every round's traversal, [25] the most nodes of one traversal, [26] traversals
// with a triangle hit, [27] the deepest level reached (rt_max_tree_depth), [28] lanes whose walk overflowed,
// [29] traversals (rounds summed over the rays: rt_n_total_rays).
constexpr uint32_t kStatStack = 64;
__global__ __launch_bounds__(64) void k_ref_node_stats(const KArgs karg) {
    __shared__ uint32_t stack[kStatStack][64];
    __shared__ uint8_t level[kStatStack][64];
    (void)karg;
    const KArgs& K = kargs();
    const uint32_t lane = threadIdx.x, tiles_x = (K.a.width + 7) / 8;
    const uint32_t px = (blockIdx.x % tiles_x) * 8 + (lane & 7u), py = (blockIdx.x / tiles_x) * 8 + (lane >> 3);
    const bool valid = px < K.a.width && py < K.a.height;
    uint32_t nodes = 0, depth = 0, hits = 0, rounds = 0, over = 0;
    if (valid) {
        float o[3], d[3];
        gen_ray(K.ubo, (float)px, (float)py, o, d);
        const ObjRay R = make_obj_ray(d);
        const size_t pix = (size_t)py * K.a.width + px;
        const float tri = K.a.tri_t ? K.a.tri_t[pix] : kTMax;
        const float tcut = tri * R.norm;
        uint4 rs = reinterpret_cast<uint4*>(K.a.ray_stats)[pix];
        rounds = rs.z;
        auto enter = [&](const float lo[3], const float hi[3]) {
            float l0 = (lo[0] - o[0]) * R.idir[0], h0 = (hi[0] - o[0]) * R.idir[0];
            float l1 = (lo[1] - o[1]) * R.idir[1], h1 = (hi[1] - o[1]) * R.idir[1];
            float l2 = (lo[2] - o[2]) * R.idir[2], h2 = (hi[2] - o[2]) * R.idir[2];
            float t = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(l0, h0), R.tmin),
                                      __builtin_fmaxf(__builtin_fminf(l1, h1), __builtin_fminf(l2, h2)));
            float u = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(l0, h0), R.tmax),
                                      __builtin_fminf(__builtin_fmaxf(l1, h1), __builtin_fmaxf(l2, h2)));
            return t <= u && t < tcut;
        };
        if (K.a.n == 1) {
            nodes = 1;  // the root is the only leaf
            depth = 1;
        } else if (K.a.n > 1) {
            uint32_t sp = 0;
            stack[sp][lane] = K.a.root_ref;
            level[sp++][lane] = 1;
            while (sp) {
                --sp;
                const uint32_t ref = stack[sp][lane], lv = level[sp][lane];
                ++nodes;  // an internal node visited
                depth = depth > lv ? depth : lv;
                const BvhNode& nd = K.a.nodes[ref];
                const uint32_t refs[2] = {nd.l_ref, nd.r_ref};
                const float* los[2] = {nd.l_lo, nd.r_lo};
                const float* his[2] = {nd.l_hi, nd.r_hi};
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (!enter(los[c], his[c])) continue;
                    if (refs[c] & kLeafBit) {
                        ++nodes;  // a leaf reached (a candidate)
                        depth = depth > lv + 1 ? depth : lv + 1;
                    } else if (sp < kStatStack) {
                        stack[sp][lane] = refs[c];
                        level[sp++][lane] = (uint8_t)(lv + 1 < 255 ? lv + 1 : 255);
                    } else {
                        over = 1;
                    }
                }
            }
        }
        hits = tri < kTMax ? rounds : 0u;
        rs.y = hits;
        rs.w = nodes;
        reinterpret_cast<uint4*>(K.a.ray_stats)[pix] = rs;
    }
    const unsigned long long tot = wave_sum(valid ? nodes * rounds : 0u), th = wave_sum(valid ? hits : 0u);
    const unsigned long long nr = wave_sum(valid ? rounds : 0u);
    uint32_t mx = nodes, md = depth;
    for (int off = 32; off > 0; off >>= 1) {
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
        md = max(md, (uint32_t)__shfl_xor((int)md, off));
    }
    const bool ov = __ballot(over != 0) != 0;
    if (lane == 0) {
        unsigned long long* c = K.a.counters;
        atomicAdd(c + 24, tot);
        atomicMax(c + 25, (unsigned long long)mx);
        atomicAdd(c + 26, th);
        atomicMax(c + 27, (unsigned long long)md);
        if (ov) atomicAdd(c + 28, 1ull);
        atomicAdd(c + 29, nr);
    }
}

// ----------------------------------------------------------------------------------------- host side

uint32_t max_local_tiles(const RenderPlan& p) {  // the packed stride of the gather: the largest share
    uint32_t m = 0;
    for (uint32_t r = 0; r < p.nranks; ++r) {
        const uint32_t n = p.tiles_x * (p.bands.row[r + 1] - p.bands.row[r]);
        m = n > m ? n : m;
    }
    return m;
}

// GSRT_DEBUG_NO_FRONTIER=1: groups traverse from the root (A/B measurements, tests)
static bool debug_no_frontier() {
    const char* e = std::getenv("GSRT_DEBUG_NO_FRONTIER");
    return e && e[0] == '1';
}

// GSRT_DEBUG_PROJECT_ALL=1: a rank of a sharded frame keeps every splat in its projection (A/B, tests)
static bool debug_project_all() {
    const char* e = std::getenv("GSRT_DEBUG_PROJECT_ALL");
    return e && e[0] == '1';
}

// GSRT_DEBUG_NO_GROUPS=1: no group lists, every tile traverses the BVH itself (A/B measurements, tests)
static bool debug_no_groups() {
    const char* e = std::getenv("GSRT_DEBUG_NO_GROUPS");
    return e && e[0] == '1';
}

// test / A-B knob: COR traversals test the leaf AABBs and cull footprints from the footprint array, as before leaf_fp
static bool debug_no_leaf_fp() {
    const char* e = std::getenv("GSRT_DEBUG_NO_LEAF_FP");
    return e && e[0] == '1';
}

template <class V>
static void launch_cor_t(hipStream_t st, const KArgs& k) {
    hipLaunchKernelGGL((k_render_cor<V>), dim3(k.a.ntiles_local), dim3(64), 0, st, k);
}

// A rank of a sharded frame projects in sorted-leaf chunks (k_prep_cor) from this many ranks on: most 64-leaf chunks
// then lie wholly outside its band and are rejected by one box test, while its own splats are gathered by leaf.
// At 2 ranks a band is half the frame and the chunked walk costs more than it saves (profiles/r05/leaf_ab.txt)
constexpr uint32_t kLeafOrderRanks = 4;

// Grow one slot buffer (only on the first frame of a geometry: both streams are drained first, since the old
// buffer may still be read by either of them).
template <class T>
static gsrt_status grow_slot(gsrt_ctx* ctx, T** p, size_t bytes) {
    (void)hipFree(*p);
    *p = nullptr;
    GSRT_HIP(ctx, hipMalloc(p, bytes));
    return GSRT_OK;
}

// The prep streams' priority class from the sampled render kernel time (kPrioLowAboveUs). A switch makes the new
// pair wait for everything queued on the old one, so stream order carries over; events recorded on the old
// streams stay valid.
static void choose_prep_priority(gsrt_ctx* ctx) {
    // test switch GSRT_DEBUG_PREP_PRIORITY: 0 / 1 forced low / high (at creation), 2 switch at every frame
    const char* e = std::getenv("GSRT_DEBUG_PREP_PRIORITY");
    if (e && (e[0] == '0' || e[0] == '1')) return;
    const bool flip = e && e[0] == '2';
    if (!flip && ctx->render_us < 0.0f) return;  // no render kernel time sampled yet
    bool high = ctx->prep_high;
    if (flip) high = !high;
    else if (high && ctx->render_us > kPrioLowAboveUs) high = false;
    else if (!high && ctx->render_us < kPrioHighBelowUs) high = true;
    if (high == ctx->prep_high) return;
    hipStream_t* to = high ? ctx->prep_hi : ctx->prep_lo;
    hipStream_t* from = high ? ctx->prep_lo : ctx->prep_hi;
    for (uint32_t j = 0; j < kStreamSlots; ++j) {
        if (hipEventRecord(ctx->ev_hop[j], from[j]) != hipSuccess || hipStreamWaitEvent(to[j], ctx->ev_hop[j], 0) != hipSuccess) {
            // the old set cannot be waited for by event: drain it instead
            (void)hipGetLastError();
            for (uint32_t i = 0; i < kStreamSlots; ++i) (void)hipStreamSynchronize(from[i]);
        }
    }
    ctx->pstream = to[0];
    ctx->fstream = to[1];
    ctx->prep_high = high;
}

// frame slots in rotation: three, so that a frame's prep (a moving scene's refit, projection and group lists) may start
// while the two frames before it still render; two on slot streams (one slot per prep stream).
// Test switch GSRT_DEBUG_SLOTS=2: always two.
static uint32_t choose_slots(bool slot_streams) {
    const char* e = std::getenv("GSRT_DEBUG_SLOTS");
    return slot_streams || (e && e[0] == '2') ? 2u : kSlots;
}

bool use_slot_streams(gsrt_ctx* ctx, bool share) {
    for (uint32_t j = 0; j < kSlots; ++j) {
        FrameSlot& S = ctx->slot[j];
        if (!S.timed || hipEventQuery(S.t1) != hipSuccess) continue;  // not sampled, or still running
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, S.t0, S.t1) == hipSuccess) ctx->render_us = ms * 1e3f;
        S.timed = false;
    }
    (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady
    choose_prep_priority(ctx);
    if (const char* e = std::getenv("GSRT_DEBUG_SLOT_STREAMS"))  // test knob: 0 never, 1 always
        if (e[0] == '0' || e[0] == '1') return e[0] == '1';
    if (ctx->render_us >= 0.0f) {
        const float enter = share ? kSlotEnterUs : kSlotEnterUsFrame, leave = share ? kSlotLeaveUs : kSlotLeaveUsFrame;
        if (!ctx->slot_mode && ctx->render_us < enter) ctx->slot_mode = true;
        else if (ctx->slot_mode && ctx->render_us > leave) ctx->slot_mode = false;
    }
    return ctx->slot_mode;
}

// ---- launch_render: one frame's launches, as a sequence of phases over what the frame is (FramePath)

// What a frame is: its slot and streams, and which prep path it goes down. Fixed once (frame_path) from the plan, the
// caller's RenderSync, the context and the scene; the phases below read it and none of them decides again.
struct FramePath {
    bool cor, stats;
    // COR frames rotate over the kSlots frame slots, their prep kernels on the prep stream; REF and the counting pass
    // run everything on the render stream in slot 0, ordered after all earlier prep work
    bool pipelined;
    // slot streams (use_slot_streams, gsrt_internal.hpp): the frame's prep and render kernels on its slot's stream
    bool slot_streams;
    uint32_t b, prev;   // the frame's slot, and the slot of the frame before this one
    hipStream_t ps;     // the stream of the prep kernels
    bool use_groups;    // k_group_list builds the tile lists (else k_collect_cor per tile)
    bool frontier;      // the groups traverse from their super-group's frontier (else from the root)
    bool leaf_fp;       // the projection writes each leaf's footprint box into its node
    // a rank of a sharded COR frame: its projection keeps only what its band can see, its frontier kernel skips the
    // super-groups outside the band
    RankTiles own;
    // the fused prep head (k_prep_cor: frontier + projection in one launch) for pipelined COR frames; otherwise the
    // frontier runs on its own stream beside the projection (two short latency chains in parallel), except on slot
    // streams
    bool fused;
    // a rank share projects in sorted-leaf chunks (k_prep_cor, kLeafOrderRanks): the slot's keyed bitmap follows the
    // order (switching it starts the bitmap over: all ones, every key rewritten once)
    bool leaf_order;
    // a pipelined rank share: the slot's in-band bitmap for this camera and band (k_classify, once per AABB version and
    // key), which its fit and projection read instead of the AABBs of the splats the band cannot see
    bool band_frame;
};

// (also takes the frame's slot: fixes the rotation's length for this frame, ctx->nslots)
static FramePath frame_path(gsrt_scene* sc, const gsrt_ubo& ubo, const RenderPlan& plan, const RenderSync* sync) {
    gsrt_ctx* ctx = sc->ctx;
    FramePath f{};
    f.stats = (plan.mode & GSRT_FLAG_STATS) != 0;
    f.cor = (plan.mode & 0xffu) == GSRT_MODE_COR;
    f.pipelined = f.cor && !f.stats;
    f.slot_streams = f.pipelined && sync && sync->slot && sync->private_out;
    f.prev = ctx->prev_slot;
    if (f.pipelined) ctx->nslots = choose_slots(f.slot_streams);
    if (f.pipelined && ctx->next_slot >= ctx->nslots) ctx->next_slot = 0;  // (the rotation shrank: never the last slot)
    f.b = f.pipelined ? ctx->next_slot : 0u;
    f.ps = f.pipelined ? (f.slot_streams ? slot_stream(ctx, f.b) : ctx->pstream) : ctx->stream;
    if (local_tiles(plan) == 0) return f;  // a band without rows launches nothing: no path to choose, no switch read
    f.use_groups = f.cor && sc->n > 1 && !f.stats && !debug_no_groups();
    f.frontier = f.use_groups && !debug_no_frontier();
    f.leaf_fp = f.cor && !f.stats && sc->n >= 2 && !debug_no_leaf_fp();
    if (f.cor && !f.stats && plan.nranks > 1 && !debug_project_all())
        f.own = RankTiles{1u, (float)(plan.row0() * plan.th), (float)(plan.row1() * plan.th), (float)ubo.width};
    f.fused = f.pipelined && f.frontier && sc->n >= 2;
    f.leaf_order = f.fused && f.own.active && plan.nranks >= kLeafOrderRanks;
    f.band_frame = f.pipelined && f.own.active && sc->n >= 2;
    return f;
}

// scene updates go on pstream: a frame on another slot stream follows those queued so far, and the next update's
// copies wait for this frame (order_update)
static gsrt_status follow_updates(gsrt_ctx* ctx, const FramePath& f) {
    if (!f.slot_streams || f.b == 0) return GSRT_OK;
    if (ctx->side_updates[f.b]) {
        GSRT_HIP(ctx, hipEventRecord(ctx->ev_fit, ctx->pstream));
        GSRT_HIP(ctx, hipStreamWaitEvent(f.ps, ctx->ev_fit, 0));
        ctx->side_updates[f.b] = false;
    }
    ctx->side_frames[f.b] = true;
    return GSRT_OK;
}

// Everything of the kernels' arguments that the plan, the camera, the caller's RenderSync and the scene decide. The
// buffers a frame may have to grow first are bound by the ensure_* phases, each its own.
static void fill_args(KArgs& k, const gsrt_scene* sc, const gsrt_ubo& ubo, const RenderPlan& plan, float* d_out,
                      gsrt_raystate* d_rs, const RenderSync* sync, const FramePath& f) {
    const gsrt_ctx* ctx = sc->ctx;
    std::memset(&k, 0, sizeof k);
    k.ubo = ubo;
    RenderArgs& A = k.a;
    A.sh = sc->d_sh;
    A.nodes = sc->d_nodes[f.b];
    A.lut = ctx->d_lut;
    A.out = d_out;
    A.rs = d_rs;
    // the second outputs of a whole COR frame on the in-order path (RenderSync); frames without a RenderSync (those
    // that write ray states, a one-rank sharded frame without a communicator) carry none, and no sampled render time
    const bool outputs = f.cor && !f.stats && !plan.packed && sync;
    A.depth_out = outputs ? sync->depth : nullptr;
    A.feat_out = outputs ? sync->feat : nullptr;
    A.feat_rows = A.feat_out ? sc->d_feat_rows : nullptr;
    A.feat_channels = A.feat_out ? sc->feat_channels : 0u;
    // (an SH gradient frame of a scene without SH rows is refused before it gets here, frame_refusal)
    const bool grad = outputs && sync->grad_rows && !A.depth_out && !A.feat_out &&
                      (!grad_flag(sync->grad_kind).needs_sh || sc->d_sh);
    A.grad_in = grad ? sync->grad_in : nullptr;
    A.grad_rows = grad ? sync->grad_rows : nullptr;
    A.grad_channels = grad ? sync->grad_channels : 0u;
    A.grad_depth_in = grad ? sync->grad_depth_in : nullptr;
    A.ray_stats = f.stats ? ctx->d_ray_stats : nullptr;
    A.counters = ctx->d_counters;
    A.n = sc->n;
    A.root_ref = sc->root_ref;
    A.root_box = sc->d_root_box[f.b];
    A.width = ubo.width; A.height = ubo.height;
    A.tiles_x = plan.tiles_x;
    A.tiles_y = plan.tiles_y;
    A.ntiles_local = local_tiles(plan);
    A.rank = plan.rank; A.nranks = plan.nranks; A.row0 = plan.row0(); A.row1 = plan.row1();
    if (sync && sync->dump8) {
        A.dump8 = 1u;
        A.esc = sync->esc;
        A.esc_cap = sync->esc_cap;
        A.accum = sync->accum;
    }
    A.tw = plan.tw; A.th = plan.th; A.s_lanes = plan.s_lanes; A.passes = plan.passes;
    A.packed = plan.packed ? 1u : 0u;
    A.samples = ubo.samples; A.bounces = ubo.bounces;
    A.stack_limit = kStack;
    if (const char* e = std::getenv("GSRT_DEBUG_STACK_LIMIT")) {  // test knob: exercise the DFS restart
        const long v = std::strtol(e, nullptr, 10);
        if (v >= 8 && v < (long)kStack) A.stack_limit = (uint32_t)v;
    }
    A.use_groups = f.use_groups;
    if (f.use_groups) {
        A.fg = plan.fg;
        A.groups_x = (A.tiles_x + A.fg - 1) / A.fg;
        A.groups = A.groups_x * ((A.tiles_y + A.fg - 1) / A.fg);
        if (f.frontier) {
            A.sgroups_x = (A.groups_x + kSG - 1) / kSG;
            A.sgroups = A.sgroups_x * ((A.groups / A.groups_x + kSG - 1) / kSG);
        }
    }
    // the counting pass keeps every AABB candidate (|C_r| of SURVEY.md 8d); the prep kernels do not read it
    A.cull2d = f.cor && !f.stats ? 1u : 0u;
    A.leaf_fp = f.leaf_fp ? 1u : 0u;
    A.own = f.own;
    A.depth_unsafe = sc->d_flags;
    // the depth cull pays where group lists overflow: groups of many samples per pixel (C5) or 32 pixels wide (C2, C4);
    // on the smaller groups of C3 and the 8-rank shares its tests cost more than they cull (profiles/r06/depth_cull_ab.txt)
    A.depth_cull = A.s_lanes >= kMoreLanes || plan.fg * plan.tw >= 32 ? 1u : 0u;
}

// (Re)allocation of the slots' buffers: only on the first frame of a scene / frame geometry, so simply drain every
// stream first. Every slot is sized at once: a lazily grown second slot would drain the pipeline again on the next
// frame. Then the frame's slot is bound.
static gsrt_status ensure_slot_buffers(gsrt_scene* sc, const FramePath& f, RenderArgs& A) {
    gsrt_ctx* ctx = sc->ctx;
    if (f.cor) {
        auto slot_short = [&](uint32_t j) {
            const FrameSlot& Sj = ctx->slot[j];
            return Sj.list_tiles < A.ntiles_local || (A.use_groups && Sj.group_cap < A.groups) ||
                   (A.sgroups && Sj.frontier_cap < A.sgroups) || (sc->n && (!sc->d_recs[j] || !sc->d_footprint[j]));
        };
        const uint32_t nslots = f.pipelined ? ctx->nslots : 1u;
        bool any_short = false;
        for (uint32_t j = 0; j < nslots; ++j) any_short = any_short || slot_short(j);
        if (any_short) {
            gsrt_status s = sync_all(ctx);
            if (s != GSRT_OK) return s;
            for (uint32_t j = 0; j < nslots; ++j) {
                FrameSlot& Sj = ctx->slot[j];
                if (Sj.list_tiles < A.ntiles_local) {
                    Sj.list_tiles = 0;
                    if ((s = grow_slot(ctx, &Sj.d_lists, sizeof(uint32_t) * kCap * A.ntiles_local)) != GSRT_OK ||
                        (s = grow_slot(ctx, &Sj.d_list_hdr, sizeof(uint4) * A.ntiles_local)) != GSRT_OK)
                        return s;
                    Sj.list_tiles = A.ntiles_local;
                }
                if (A.use_groups && Sj.group_cap < A.groups) {
                    Sj.group_cap = 0;
                    if ((s = grow_slot(ctx, &Sj.d_glist, sizeof(uint64_t) * kGStride * A.groups)) != GSRT_OK ||
                        (s = grow_slot(ctx, &Sj.d_ghdr, sizeof(uint4) * A.groups)) != GSRT_OK)
                        return s;
                    Sj.group_cap = A.groups;
                }
                if (A.sgroups && Sj.frontier_cap < A.sgroups) {
                    Sj.frontier_cap = 0;
                    if ((s = grow_slot(ctx, &Sj.d_frontier, sizeof(uint32_t) * (kFront + 1) * A.sgroups)) != GSRT_OK) return s;
                    Sj.frontier_cap = A.sgroups;
                }
                if (sc->n && !sc->d_recs[j]) {
                    GSRT_HIP(ctx, hipMalloc(&sc->d_recs[j], sizeof(SplatRec) * sc->n));
                    GSRT_HIP(ctx, hipMalloc(&sc->d_keyed[j], sizeof(uint32_t) * ((sc->n + 31) / 32 + 1)));
                    GSRT_HIP(ctx, hipMemset(sc->d_keyed[j], 0xFF, sizeof(uint32_t) * ((sc->n + 31) / 32 + 1)));
                }
                if (sc->n && !sc->d_footprint[j]) GSRT_HIP(ctx, hipMalloc(&sc->d_footprint[j], kFpWords * sizeof(float4) * sc->n));
            }
        }
        const FrameSlot& S = ctx->slot[f.b];
        A.lists = S.d_lists;
        A.list_hdr = reinterpret_cast<uint4*>(S.d_list_hdr);
        if (A.use_groups) {
            A.glist = reinterpret_cast<uint64_t*>(S.d_glist);
            A.ghdr = reinterpret_cast<uint4*>(S.d_ghdr);
            if (A.sgroups) A.frontier = S.d_frontier;
        }
    } else if (sc->n && !sc->d_recs[0]) {
        GSRT_HIP(ctx, hipMalloc(&sc->d_recs[0], sizeof(SplatRec) * sc->n));
    }
    A.recs = sc->d_recs[f.b];
    A.footprint = f.cor ? sc->d_footprint[f.b] : nullptr;
    return GSRT_OK;
}

// k_group_list's dispatch order (group_order, gsrt_plan.cpp), rebuilt when the group grid or the rank's band changes
static gsrt_status ensure_group_order(gsrt_ctx* ctx, RenderArgs& A) {
    const uint32_t key[5] = {A.groups_x, A.groups, A.row0, A.row1, A.nranks};
    if (std::memcmp(key, ctx->group_order_key, sizeof key) != 0) {
        gsrt_status s = sync_all(ctx);
        if (s != GSRT_OK) return s;
        std::vector<uint32_t> ord;
        ctx->group_own = group_order(A.groups_x, A.groups / A.groups_x, A.fg, A.row0, A.row1, A.nranks, ord);
        (void)hipFree(ctx->d_group_order);
        ctx->d_group_order = nullptr;
        ctx->group_order_key[0] = ctx->group_order_key[1] = 0;
        GSRT_HIP(ctx, hipMalloc(&ctx->d_group_order, sizeof(uint32_t) * A.groups));
        GSRT_HIP(ctx, hipMemcpy(ctx->d_group_order, ord.data(), sizeof(uint32_t) * A.groups, hipMemcpyHostToDevice));
        std::memcpy(ctx->group_order_key, key, sizeof key);
    }
    A.group_order = ctx->d_group_order;
    return GSRT_OK;
}

// k_render_cor's dispatch order of a rank of a sharded frame: its units of kDeal local tiles of the complete XCD rounds
// centre-out (unit_order_centre, gsrt_plan.cpp). When the context has rendered a whole COR frame of this tile grid, its
// measured tile costs order the units instead: longest first, each to the least-loaded XCD (deal_units; 8-rank C3 shares
// 0.3-6 % faster, C4 even: profiles/r06/deal_ab.txt; test switch GSRT_DEBUG_DEAL=0 keeps centre-out). One device keeps
// the spatial order (C3 -2 %, C2 -2 %, C4 +1.5 % with it).
static gsrt_status ensure_run_order(gsrt_ctx* ctx, const RenderPlan& plan, RenderArgs& A) {
    const uint32_t nl = A.ntiles_local, R = (nl / (kXcds * kDeal)) * kXcds;
    if (R <= 1) return GSRT_OK;
    const uint32_t key[5] = {nl, plan.row0(), plan.row1(), plan.tiles_x, plan.tiles_y};
    if (std::memcmp(key, ctx->run_order_key, sizeof key) != 0) {
        gsrt_status s = sync_all(ctx);
        if (s != GSRT_OK) return s;
        std::vector<uint32_t> perm(R);
        unit_order_centre(R, plan.row0(), plan.row1(), plan.tiles_x, perm.data());
        const char* de = std::getenv("GSRT_DEBUG_DEAL");
        if (!(de && de[0] == '0') && ctx->tile_cost_tx == plan.tiles_x && ctx->tile_cost_ty == plan.tiles_y) {
            // a whole frame's measured tile costs (its last one on this context)
            std::vector<uint32_t> t((size_t)plan.tiles_x * plan.tiles_y);
            GSRT_HIP(ctx, hipMemcpy(t.data(), ctx->d_tile_cost[ctx->tile_cost_slot], sizeof(uint32_t) * t.size(),
                                    hipMemcpyDeviceToHost));
            std::vector<double> uc(R);
            unit_costs(t.data(), R, plan.row0(), plan.row1(), plan.tiles_x, plan.tiles_y, uc.data());
            const std::vector<uint32_t> centre(perm);
            deal_units(uc.data(), centre.data(), R, perm.data());
        }
        (void)hipFree(ctx->d_run_order);
        ctx->d_run_order = nullptr;
        std::memset(ctx->run_order_key, 0, sizeof ctx->run_order_key);
        GSRT_HIP(ctx, hipMalloc(&ctx->d_run_order, sizeof(uint32_t) * R));
        GSRT_HIP(ctx, hipMemcpy(ctx->d_run_order, perm.data(), sizeof(uint32_t) * R, hipMemcpyHostToDevice));
        std::memcpy(ctx->run_order_key, key, sizeof key);
    }
    A.run_order = ctx->d_run_order;
    return GSRT_OK;
}

// Ordering of the prep stage: after every scene change queued on the render stream (update, refit, build), and after
// the render that last read this slot (frame f-2); not after the render of frame f-1. Takes the slot out of the rotation.
static gsrt_status order_prep(gsrt_ctx* ctx, const FramePath& f) {
    const hipStream_t st = ctx->stream, ps = f.ps;
    const FrameSlot& S = ctx->slot[f.b];
    if (f.pipelined) {
        // one flag per prep stream
        bool& dirty = ps == ctx->pstream ? ctx->main_dirty : ctx->main_dirty_f;
        if (dirty) {
            GSRT_HIP(ctx, hipEventRecord(ctx->ev_main, st));
            GSRT_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_main, 0));
            dirty = false;
        }
        // (on slot streams the slot's last render kernel is on ps already, unless it ran without them)
        if (S.render_pending && (!f.slot_streams || S.rstream != ps)) GSRT_HIP(ctx, hipStreamWaitEvent(ps, S.rendered, 0));
        if (gsrt_status su = wait_updates(ctx, ps); su != GSRT_OK) return su;  // the arrays' update copies
        ++ctx->frame_no;
        ctx->prev_slot = f.b;
        ctx->next_slot = (f.b + 1) % ctx->nslots;
    } else {
        // everything on the render stream, after all prep work issued so far (both prep streams: with slot
        // streams, frames run on fstream too); the next prep waits for it, and so do scene updates and refits
        // (their copies run on the prep stream: serial_pending)
        GSRT_HIP(ctx, hipEventRecord(ctx->ev_main, ctx->pstream));
        GSRT_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_main, 0));
        GSRT_HIP(ctx, hipEventRecord(ctx->ev_front, ctx->fstream));
        GSRT_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_front, 0));
        mark_main_dirty(ctx);
        ctx->serial_pending = true;
        ctx->serial_reads = true;  // an update retiring the arrays' buffers records this stream's position
        if (gsrt_status su = wait_updates(ctx, st); su != GSRT_OK) return su;
    }
    return GSRT_OK;
}

// The frame's tile cost profile (RenderArgs::tile_cost): a sharded frame's goes where the caller says (gsrt_comm.cpp:
// its profile frames), a whole COR frame's into the slot's own buffer (gsrt_row_costs)
static gsrt_status ensure_tile_cost(gsrt_ctx* ctx, const RenderPlan& plan, const RenderSync* sync, const FramePath& f,
                                    RenderArgs& A) {
    if (sync && sync->sharded) {
        A.tile_cost = sync->tile_cost;
    } else if (f.cor) {
        const uint32_t nt = plan.tiles_x * plan.tiles_y;
        if (ctx->tile_cost_cap < nt) {
            gsrt_status s = sync_all(ctx);
            if (s != GSRT_OK) return s;
            ctx->tile_cost_cap = 0;
            for (uint32_t j = 0; j < kSlots; ++j)
                if ((s = grow_slot(ctx, &ctx->d_tile_cost[j], sizeof(uint32_t) * nt)) != GSRT_OK) return s;
            ctx->tile_cost_cap = nt;
        }
        A.tile_cost = ctx->d_tile_cost[f.b];
        ctx->tile_cost_slot = f.b;
        ctx->tile_cost_tx = plan.tiles_x;
        ctx->tile_cost_ty = plan.tiles_y;
    }
    return GSRT_OK;
}

// The prep head on the prep stream: the slot's bitmaps, its boxes fitted if stale, then the projection and (COR with
// group lists) the super-groups' frontiers. fr: the stream the frontier went on when it runs beside the projection
// (launch_lists joins it), else ps.
static gsrt_status launch_prep(gsrt_scene* sc, const gsrt_ubo& ubo, const RenderPlan& plan, const FramePath& f,
                               const KArgs& k, hipStream_t& fr) {
    gsrt_ctx* ctx = sc->ctx;
    const RenderArgs& A = k.a;
    const uint32_t b = f.b;
    const hipStream_t ps = f.ps;
    fr = ps;
    uint32_t* keyed = f.pipelined ? sc->d_keyed[b] : nullptr;
    if (keyed && sc->slot_keyed_leaf[b] != f.leaf_order) {
        GSRT_HIP(ctx, hipMemsetAsync(keyed, 0xFF, sizeof(uint32_t) * ((sc->n + 31) / 32 + 1), ps));
        sc->slot_keyed_leaf[b] = f.leaf_order;
    }
    const FitBandKey bkey = f.band_frame ? make_band_key(ubo, f.own) : FitBandKey{};
    if (f.band_frame) {
        if (!sc->d_inband[b]) GSRT_HIP(ctx, hipMalloc(&sc->d_inband[b], sizeof(uint32_t) * ((sc->n + 31) / 32 + 1)));
        if (sc->slot_inband_ver[b] != sc->aabb_version || !same_key(bkey, sc->slot_inband_key[b])) {
            hipLaunchKernelGGL(k_classify, dim3((sc->n + 255) / 256), dim3(64), 0, ps, sc->n, ubo, f.own, sc->d_aabbs,
                               sc->d_inband[b]);
            sc->slot_inband_ver[b] = sc->aabb_version;
            sc->slot_inband_key[b] = bkey;
        }
    }
    // the slot's boxes, fitted to the current geometry if a refit came since (on the stream of the prep kernels). A
    // rank share fits only what its band can see (FitBand: the 256-leaf chunks without a splat in its bitmap get empty
    // boxes; its projection gives their splats +inf keys anyway). COR frames put each leaf's footprint box into its node
    // (leaf_fp); REF and counting frames need the AABBs there, which the slot's fit restores
    {
        const FitBand fb{f.band_frame ? sc->d_inband[b] : nullptr};
        if (gsrt_status fs = lbvh_fit_if_stale(sc, b, ps, !f.leaf_fp, f.band_frame ? &fb : nullptr,
                                               f.band_frame ? &bkey : nullptr);
            fs != GSRT_OK)
            return fs;
    }
    sc->last_slot = b;
    if (f.fused) {
        const ProjArgs pa{sc->n, sc->d_params, sc->d_aabbs, sc->d_recs[b], sc->d_nodes[b], sc->d_gid_slot,
                          sc->d_footprint[b], ctx->d_counters, f.own, keyed, A.leaf_fp,
                          f.leaf_order ? sc->d_leaf_gid : nullptr, f.band_frame ? sc->d_inband[b] : nullptr,
                          sc->d_flags};
        hipLaunchKernelGGL(k_prep_cor, dim3(A.sgroups + (sc->n + 63) / 64), dim3(64), 0, ps, k, pa);
    } else if (!f.slot_streams && f.pipelined && A.frontier) {
        // the BVH frontier needs only the camera and the fitted boxes: it runs on its own stream beside the projection
        fr = ctx->fstream;
        GSRT_HIP(ctx, hipEventRecord(ctx->ev_fit, ps));
        GSRT_HIP(ctx, hipStreamWaitEvent(fr, ctx->ev_fit, 0));
        hipLaunchKernelGGL(k_frontier, dim3(A.sgroups), dim3(64), 0, fr, k);
    }
    // pipelined COR frames keep the slot's keyed bitmap; any other projection of the slot (REF, counting pass)
    // writes every record unbooked, so the bitmap goes back to all ones behind it (the next prep waits for it)
    if (!f.fused)
        launch_project(ps, sc->n, plan.mode, ubo, sc->d_params, sc->d_aabbs, sc->d_recs[b], sc->d_nodes[b],
                       sc->d_gid_slot, f.cor ? sc->d_footprint[b] : nullptr, ctx->d_counters, &f.own, keyed, f.leaf_fp,
                       sc->d_flags);
    sc->slot_leaf_fp[b] = f.leaf_fp;  // (either projection above)
    if (!f.pipelined && sc->n && sc->d_keyed[b])
        GSRT_HIP(ctx, hipMemsetAsync(sc->d_keyed[b], 0xFF, sizeof(uint32_t) * ((sc->n + 31) / 32 + 1), ps));
    return GSRT_OK;
}

// A REF frame's render kernel on the render stream, after the mesh's closest hits where the scene holds triangles
static gsrt_status launch_ref(gsrt_scene* sc, const gsrt_ubo& ubo, const RenderPlan& plan, const FramePath& f,
                              RenderSync* sync, KArgs& k) {
    gsrt_ctx* ctx = sc->ctx;
    const hipStream_t st = ctx->stream;
    if (sc->ntri) {
        const size_t px = (size_t)ubo.width * ubo.height;
        if (ctx->tri_t_pixels < px) {
            gsrt_status s = sync_all(ctx);
            if (s != GSRT_OK) return s;
            ctx->tri_t_pixels = 0;
            if ((s = grow_slot(ctx, &ctx->d_tri_t, sizeof(float) * px)) != GSRT_OK) return s;
            ctx->tri_t_pixels = px;
        }
        launch_mesh_thit(st, ubo, sc, ctx->d_tri_t);
        k.a.tri_t = ctx->d_tri_t;
    }
    if (sync && sync->wait) GSRT_HIP(ctx, hipStreamWaitEvent(st, sync->wait, 0));
    if (sync) sync->stream = st;
    timing_mark(ctx, 1);
    if (f.stats) hipLaunchKernelGGL((k_render_ref<true>), dim3(k.a.ntiles_local), dim3(64), 0, st, k);
    else hipLaunchKernelGGL((k_render_ref<false>), dim3(k.a.ntiles_local), dim3(64), 0, st, k);
    if (f.stats && k.a.ray_stats && !plan.packed)  // VS-style traversal statistics (gsrt_vs_stats)
        hipLaunchKernelGGL(k_ref_node_stats, dim3(((ubo.width + 7) / 8) * ((ubo.height + 7) / 8)), dim3(64), 0, st, k);
    timing_mark(ctx, 2);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

// The k_render_cor instantiation of a frame: every one the library holds is named here and nowhere else. Feature and
// gradient frames blend no SH whatever the scene holds (never with stats or depth, frame_refusal).
using CorLaunch = void (*)(hipStream_t, const KArgs&);
template <CorKind K>
static CorLaunch cor_kernel_of(bool sh, bool lut) {
    if constexpr (K == CorKind::feat || K == CorKind::grad)
        return lut ? launch_cor_t<CorVariant<K, false, true>> : launch_cor_t<CorVariant<K, false, false>>;
    else if constexpr (K == CorKind::shgrad)  // only for a scene with SH rows (gsrt_api.cpp: GSRT_E_STATE without)
        return lut ? launch_cor_t<CorVariant<K, true, true>> : launch_cor_t<CorVariant<K, true, false>>;
    else if constexpr (K == CorKind::splatgrad || K == CorKind::splatdepthgrad)  // never with the LUT (frame_refusal)
        return sh ? launch_cor_t<CorVariant<K, true, false>> : launch_cor_t<CorVariant<K, false, false>>;
    else
        return sh ? (lut ? launch_cor_t<CorVariant<K, true, true>> : launch_cor_t<CorVariant<K, true, false>>)
                  : (lut ? launch_cor_t<CorVariant<K, false, true>> : launch_cor_t<CorVariant<K, false, false>>);
}
static CorLaunch cor_kernel(CorKind kind, bool sh, bool lut) {
    switch (kind) {
        case CorKind::plain: return cor_kernel_of<CorKind::plain>(sh, lut);
        case CorKind::stats: return cor_kernel_of<CorKind::stats>(sh, lut);
        case CorKind::depth: return cor_kernel_of<CorKind::depth>(sh, lut);
        case CorKind::feat: return cor_kernel_of<CorKind::feat>(sh, lut);
        case CorKind::grad: return cor_kernel_of<CorKind::grad>(sh, lut);
        case CorKind::shgrad: return cor_kernel_of<CorKind::shgrad>(sh, lut);
        case CorKind::opgrad: return cor_kernel_of<CorKind::opgrad>(sh, lut);
        case CorKind::splatgrad: return cor_kernel_of<CorKind::splatgrad>(sh, lut);
        case CorKind::splatdepthgrad: return cor_kernel_of<CorKind::splatdepthgrad>(sh, lut);
    }
    return nullptr;
}

// The frame's candidate lists: the frontier joined (or run here), then the first-round lists on the prep stream beside
// the previous frame's render kernel. ls: the stream they went on.
static gsrt_status launch_lists(gsrt_ctx* ctx, const FramePath& f, const RenderSync* sync, const KArgs& k, hipStream_t fr,
                                hipStream_t& ls) {
    const RenderArgs& A = k.a;
    const hipStream_t ps = f.ps;
    if (A.frontier && fr != ps) {  // pipelined: the frontier ran beside the projection; join it here
        GSRT_HIP(ctx, hipEventRecord(ctx->ev_front, fr));
        GSRT_HIP(ctx, hipStreamWaitEvent(ps, ctx->ev_front, 0));
    } else if (A.frontier && !f.fused) {
        hipLaunchKernelGGL(k_frontier, dim3(A.sgroups), dim3(64), 0, ps, k);
    }
    // Side lists: a rank share of a moving scene (an update or refit came before this frame, and likely comes before the
    // next) runs them on the other prep stream, which idles on the two-stream scheme, so that the next frame's update
    // copies, refit and projection on the prep stream (which read and write none of this slot's lists) need not wait for
    // them: the rank's serial chain is then max(lists, copies) + fit + projection instead of their sum. The lists read
    // only this slot's nodes, records and footprints, and the render kernel waits for them through `prepared` (recorded
    // there)
    const bool side_lists = f.pipelined && !f.slot_streams && sync && sync->sharded && ctx->scene_moved && A.use_groups &&
                            ps == ctx->pstream;
    ls = ps;
    if (side_lists) {
        ls = ctx->fstream;
        GSRT_HIP(ctx, hipEventRecord(ctx->ev_lists, ps));
        GSRT_HIP(ctx, hipStreamWaitEvent(ls, ctx->ev_lists, 0));
    }
    if (f.pipelined) ctx->scene_moved = false;
    if (A.use_groups) {
        // only the groups with a tile of this rank's band (the head of group_order); the others would return at once
        const uint32_t ng = std::max(1u, std::min(ctx->group_own, A.groups));
        if (A.fg == 2) hipLaunchKernelGGL(k_group_list<2>, dim3(ng), dim3(64), 0, ls, k);
        else hipLaunchKernelGGL(k_group_list<kFG>, dim3(ng), dim3(64), 0, ls, k);
        for (uint32_t seg = 1; seg < kGSegs && A.s_lanes >= kMoreLanes; ++seg) {
            if (A.fg == 2) hipLaunchKernelGGL(k_group_more<2>, dim3(ng), dim3(64), 0, ls, k);
            else hipLaunchKernelGGL(k_group_more<kFG>, dim3(ng), dim3(64), 0, ls, k);
        }
    }
    else hipLaunchKernelGGL(k_collect_cor, dim3(A.ntiles_local), dim3(64), 0, ps, k);
    GSRT_HIP(ctx, hipGetLastError());
    return GSRT_OK;
}

// The render kernel: on the render stream after the lists (cross-stream), or (slot streams) on the slot's stream right
// behind them, after the previous frame's render kernel (cross-stream); then the slot's `rendered` bookkeeping
static gsrt_status launch_cor(gsrt_scene* sc, const RenderPlan& plan, const FramePath& f, RenderSync* sync, KArgs& k,
                              hipStream_t ls) {
    gsrt_ctx* ctx = sc->ctx;
    const hipStream_t st = ctx->stream;
    FrameSlot& S = ctx->slot[f.b];
    const RenderArgs& A = k.a;
    CorKind kind = A.feat_out ? CorKind::feat : A.depth_out ? CorKind::depth : f.stats ? CorKind::stats : CorKind::plain;
    if (A.grad_rows)
        switch (sync->grad_kind) {
            case GradKind::opacity: kind = CorKind::opgrad; break;
            case GradKind::splat: kind = CorKind::splatgrad; break;
            case GradKind::splat_depth: kind = CorKind::splatdepthgrad; break;
            case GradKind::sh: kind = CorKind::shgrad; break;
            default: kind = CorKind::grad; break;
        }
    const CorLaunch render = cor_kernel(kind, sc->d_sh != nullptr, (plan.mode & GSRT_FLAG_LUT) != 0);
    hipStream_t rs = st;
    if (f.slot_streams) {
        rs = f.ps;
        const FrameSlot& O = ctx->slot[f.prev];
        if (O.render_pending && !(sync && sync->private_out)) GSRT_HIP(ctx, hipStreamWaitEvent(rs, O.rendered, 0));
    } else if (f.pipelined) {
        GSRT_HIP(ctx, hipEventRecord(S.prepared, ls));
        GSRT_HIP(ctx, hipStreamWaitEvent(st, S.prepared, 0));
    }
    if (sync && sync->wait) GSRT_HIP(ctx, hipStreamWaitEvent(rs, sync->wait, 0));
    if (sync) sync->stream = rs;
    k.a.prelisted = 1;
    // sampled render kernel time for the slot-stream and prep-priority decisions (use_slot_streams)
    const bool sample = f.pipelined && sync && !S.timed && ctx->frame_no % kTimedEvery == 1 &&
                        S.t0 && S.t1;
    if (sample) GSRT_HIP(ctx, hipEventRecord(S.t0, rs));
    timing_mark(ctx, 1, rs);  // the timed kernel is the shading/continuation kernel k_render_cor
#ifdef GSRT_WAVE_TIMES
    hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, rs, 0u);
#endif
    render(rs, k);
#ifdef GSRT_WAVE_TIMES
    hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, rs, 1u);
#endif
    GSRT_HIP(ctx, hipGetLastError());
    timing_mark(ctx, 2, rs);
    if (sample) {
        GSRT_HIP(ctx, hipEventRecord(S.t1, rs));
        S.timed = true;
    }
    if (f.pipelined) {
        GSRT_HIP(ctx, hipEventRecord(S.rendered, rs));
        S.render_pending = true;
        S.rstream = rs;
    }
    ctx->last_slot_streams = f.slot_streams;
    // whatever follows on the render stream (copies, gathers, downloads) comes after this frame
    if (f.slot_streams) GSRT_HIP(ctx, hipStreamWaitEvent(st, S.rendered, 0));
    return GSRT_OK;
}

gsrt_status launch_render(gsrt_scene* sc, const gsrt_ubo& ubo, const RenderPlan& plan, float* d_out,
                          gsrt_raystate* d_rs, RenderSync* sync) {
    gsrt_ctx* ctx = sc->ctx;
    if (sync) sync->stream = ctx->stream;
    const FramePath f = frame_path(sc, ubo, plan, sync);
    gsrt_status s = follow_updates(ctx, f);
    if (s != GSRT_OK) return s;
    KArgs k;
    fill_args(k, sc, ubo, plan, d_out, d_rs, sync, f);
    if (k.a.ntiles_local == 0) {  // a band without rows (fewer tile rows than ranks): nothing to render
        timing_mark(ctx, 1);
        timing_mark(ctx, 2);
        return GSRT_OK;
    }
    if ((s = ensure_slot_buffers(sc, f, k.a)) != GSRT_OK) return s;
    if (f.use_groups && (s = ensure_group_order(ctx, k.a)) != GSRT_OK) return s;
    if (f.cor && plan.nranks > 1 && (s = ensure_run_order(ctx, plan, k.a)) != GSRT_OK) return s;
    if ((s = order_prep(ctx, f)) != GSRT_OK) return s;
    if ((s = ensure_tile_cost(ctx, plan, sync, f, k.a)) != GSRT_OK) return s;
    hipStream_t fr, ls;
    if ((s = launch_prep(sc, ubo, plan, f, k, fr)) != GSRT_OK) return s;
    if (!f.cor) return launch_ref(sc, ubo, plan, f, sync, k);
    if ((s = launch_lists(ctx, f, sync, k, fr, ls)) != GSRT_OK) return s;
    return launch_cor(sc, plan, f, sync, k, ls);
}

// a band's row costs from its tiles' (k_render_cor's tile_cost, local order): one wave per row
__global__ __launch_bounds__(64) void k_row_sum(const uint32_t* __restrict__ tile_cost, uint32_t* __restrict__ row_cost,
                                               uint32_t tiles_x, uint32_t row0, uint32_t row1) {
    const uint32_t ty = row0 + blockIdx.x;
    uint32_t v = 0;
    for (uint32_t tx = threadIdx.x; tx < tiles_x; tx += 64) v += tile_cost[band_index(tx, ty, row0, row1, tiles_x)];
    v = (uint32_t)wave_sum(v);
    if (threadIdx.x == 0) row_cost[ty] = v;
}

void launch_row_sum(hipStream_t s, const uint32_t* tile_cost, uint32_t* row_cost, uint32_t tiles_x, uint32_t row0,
                    uint32_t row1) {
    if (row1 > row0) hipLaunchKernelGGL(k_row_sum, dim3(row1 - row0), dim3(64), 0, s, tile_cost, row_cost, tiles_x, row0, row1);
}

__global__ __launch_bounds__(256) void k_unpack(const float4* __restrict__ g, float4* __restrict__ fb, uint32_t W,
                                                uint32_t H, uint32_t tw, uint32_t th, uint32_t tiles_x, const Bands bands,
                                                uint32_t tiles_per_rank) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= W * H) return;
    const uint32_t x = i % W, y = i / W, tx = x / tw, ty = y / th;
    const uint32_t r = band_of(bands, ty);
    const uint32_t lt = band_index(tx, ty, bands.row[r], bands.row[r + 1], tiles_x);
    const uint32_t pin = (y % th) * tw + (x % tw);
    fb[i] = g[((size_t)r * tiles_per_rank + lt) * (tw * th) + pin];
}

__global__ __launch_bounds__(256) void k_unpack_dump8(const uint32_t* __restrict__ g, uint32_t* __restrict__ codes,
                                                      uint32_t W, uint32_t H, uint32_t tw, uint32_t th, uint32_t tiles_x,
                                                      const Bands bands, size_t block_words) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= W * H) return;
    const uint32_t x = i % W, y = i / W, tx = x / tw, ty = y / th;
    const uint32_t r = band_of(bands, ty);
    const uint32_t lt = band_index(tx, ty, bands.row[r], bands.row[r + 1], tiles_x);
    codes[i] = g[(size_t)r * block_words + (size_t)lt * (tw * th) + (y % th) * tw + (x % tw)];
}

void launch_unpack_dump8(hipStream_t s, const uint32_t* gathered, uint32_t* codes, const RenderPlan& p, uint32_t W,
                         uint32_t H, uint32_t tiles_per_rank, size_t block_words) {
    (void)tiles_per_rank;
    hipLaunchKernelGGL(k_unpack_dump8, dim3((W * H + 255) / 256), dim3(256), 0, s, gathered, codes, W, H, p.tw, p.th,
                       p.tiles_x, p.bands, block_words);
}

void launch_unpack(hipStream_t s, const float* gathered, float* fb, const RenderPlan& p, uint32_t W, uint32_t H,
                   uint32_t tiles_per_rank) {
    hipLaunchKernelGGL(k_unpack, dim3((W * H + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float4*>(gathered),
                       reinterpret_cast<float4*>(fb), W, H, p.tw, p.th, p.tiles_x, p.bands, tiles_per_rank);
}

}  // namespace gsrt

#ifdef GSRT_WAVE_TIMES
extern "C" int gsrt_diag_stamps(uint32_t* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(gsrt::g_stamps), 16, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
extern "C" int gsrt_diag_wave_times(uint32_t kind, void* out, uint32_t n) {
    if (kind > 1 || n > (1u << 18)) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(gsrt::g_wave_times), sizeof(uint4) * n, sizeof(uint4) * (1u << 18) * kind,
                               hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
