// gsrt_plan.cpp -- host arithmetic that plans a frame: the tile plan and the band partition, and the dispatch orders
// of k_group_list's groups and of a rank share's render units. Plain C++ (no HIP runtime calls): launch_render
// (gsrt_render.hip) uploads the orders, the test hooks at the end expose them to the CPU tests.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "gsrt_internal.hpp"

namespace gsrt {

// Rank 0 also lands the other N-1 blocks and unpacks the whole frame, a cost that grows with the framebuffer bytes
// (N - 1 blocks in, every pixel out) against a share's shading work (~ rays / N). Measured with the loopback stand-in
// (profiles/r04/): the 8-rank root's extra time is 0.2 of a share at C3 (4 spp) and 0.7 at C4 (1 spp), i.e. about
// 0.09 (N - 1) / spp of the root's frame; so rank 0 takes w0 = 1 - 0.09 (N - 1) / spp of a share (>= 1/4). A pure
// function of N and spp: every rank computes the same weight (no per-rank input reaches the partition).
float root_weight(uint32_t nranks, uint32_t spp, uint32_t mode) {
    if (nranks <= 1) return 1.0f;
    // the receive + unpack cost, in shares per (N - 1) / spp: measured for each exchange format (RGBA32F 16 B per
    // pixel, dump codes 4 B: not a quarter of it, since the root's receive and unpack are not bound by bytes alone;
    // the 8-rank C3 and C4 roots put it at 0.067-0.073)
    const float per_px = (mode & GSRT_FLAG_OUT_DUMP8) ? 0.07f : 0.09f;
    const float w0 = 1.0f - per_px * (float)(nranks - 1) / (float)(spp ? spp : 1);
    return w0 < 0.25f ? 0.25f : (w0 > 1.0f ? 1.0f : w0);
}

static void row_prefix(uint32_t tiles_y, const uint32_t* row_cost, std::vector<uint64_t>& P) {
    P.assign(tiles_y + 1, 0);
    for (uint32_t i = 0; i < tiles_y; ++i) P[i + 1] = P[i] + (row_cost ? (uint64_t)row_cost[i] : 1u);
}

void balance_bands(uint32_t tiles_y, uint32_t nranks, const uint32_t* row_cost, float root_w, uint32_t* out) {
    const uint32_t N = nranks ? nranks : 1;
    std::vector<uint64_t> P;
    row_prefix(tiles_y, row_cost, P);
    const double wtot = (double)root_w + (double)(N - 1);
    const uint32_t minrow = tiles_y >= N ? 1u : 0u;  // every band non-empty when there are enough rows
    out[0] = 0;
    out[N] = tiles_y;
    double wsum = 0.0;
    for (uint32_t r = 1; r < N; ++r) {
        wsum += r == 1 ? (double)root_w : 1.0;
        // the cumulative target of bands 0..r-1, met by the nearest row boundary the remaining bands leave room for
        const double target = (double)P[tiles_y] * wsum / wtot;
        const uint32_t lo = out[r - 1] + minrow, hi = tiles_y - (N - r) * minrow;
        uint32_t i = (uint32_t)(std::lower_bound(P.begin() + lo, P.begin() + hi + 1, (uint64_t)std::ceil(target)) - P.begin());
        if (i > hi) i = hi;
        if (i > lo && (double)P[i] - target > target - (double)P[i - 1]) --i;
        out[r] = i;
    }
}

double band_peak(uint32_t nranks, const uint32_t* bands, const uint32_t* row_cost, float root_w) {
    std::vector<uint64_t> P;
    row_prefix(bands[nranks], row_cost, P);
    double peak = 0.0;
    for (uint32_t r = 0; r < nranks; ++r) {
        const double c = (double)(P[bands[r + 1]] - P[bands[r]]) / (r == 0 ? (double)root_w : 1.0);
        peak = c > peak ? c : peak;
    }
    return peak;
}

RenderPlan make_plan(const gsrt_ubo& ubo, uint32_t mode, uint32_t k, uint32_t rank, uint32_t nranks,
                     const uint32_t* bands) {
    RenderPlan p;
    p.mode = mode;
    p.cap = kCap;
    (void)k;
    p.nranks = nranks ? (nranks < kMaxRanks ? nranks : kMaxRanks) : 1;
    p.rank = rank < p.nranks ? rank : 0;
    const uint32_t S = ubo.samples ? ubo.samples : 1;
    if ((mode & 0xffu) == GSRT_MODE_REF) {
        p.tw = p.th = 8; p.s_lanes = 1; p.passes = 1;
    } else if (S <= 64 && (S & (S - 1)) == 0) {
        uint32_t px = 64 / S, lg = 0;
        while ((1u << lg) < px) ++lg;
        p.tw = 1u << ((lg + 1) / 2);
        p.th = 1u << (lg / 2);
        p.s_lanes = S; p.passes = 1;
    } else {
        p.tw = p.th = 8; p.s_lanes = 1; p.passes = S;
    }
    p.tiles_x = (ubo.width + p.tw - 1) / p.tw;
    p.tiles_y = (ubo.height + p.th - 1) / p.th;
    // the partition: the given bands (a cost-balanced partition, gsrt_comm.cpp), else rows split evenly by weight
    p.bands.n = p.nranks;
    if (bands) {
        for (uint32_t r = 0; r <= p.nranks; ++r) p.bands.row[r] = bands[r];
    } else {
        const float w0 = (mode & 0xffu) == GSRT_MODE_COR ? root_weight(p.nranks, S, mode) : 1.0f;
        balance_bands(p.tiles_y, p.nranks, nullptr, w0, p.bands.row);
    }
    // tile groups: 4x4 tiles, or 2x2 when a rank would get fewer than 1500 groups of 4x4. A rank's group lists
    // are latency chains (traversal, sort, filter) beside the previous frame's render; with few groups there are
    // too few of them to fill the GPU, and smaller groups shorten each chain. Measured: C3 (8160), C4 (8160) and
    // C5 (32400) are 6-10 % faster with 4x4; the 8-rank C3 and C4 shares (1020 groups of 4x4) 15-20 % faster
    // with 2x2; C2 and the 4-rank C3 share (2040) 5-9 % faster with 4x4 since slot streams overlap their frames
    // (before them C2 was 9 % faster with 2x2; profiles/r02c/ab_group_tiles_slot.txt). The test switch
    // GSRT_DEBUG_GROUP_TILES=2|4 overrides.
    {
        const uint32_t g4 = ((p.tiles_x + kFG - 1) / kFG) * ((p.tiles_y + kFG - 1) / kFG);
        p.fg = g4 < 1500u * p.nranks ? 2u : kFG;
    }
    if (const char* e = std::getenv("GSRT_DEBUG_GROUP_TILES")) {
        const long v = std::strtol(e, nullptr, 10);
        if (v == 2 || v == (long)kFG) p.fg = (uint32_t)v;
    }
    return p;
}

// Centre-out dispatch order of k_group_list (the groups with the longest lists first, the light border groups last: the
// kernel's tail is short groups instead of the heaviest ones started late), whole super-groups (kSG x kSG groups, one
// frontier) dealt round-robin over the XCDs (workgroup i runs on XCD i % kXcds), so an XCD's consecutive groups share
// the top of the BVH in its L2. Measured at r03 (profiles/archive/r03/pmc_gorder.txt): k_group_list's C3 FETCH_SIZE
// 246 -> 139 MB per launch against single groups centre-out. A rank of a sharded frame orders (and deals) only the
// groups with a tile row of its band [row0, row1): the count returned; the others go last and are not launched.
uint32_t group_order(uint32_t groups_x, uint32_t groups_y, uint32_t fg, uint32_t row0, uint32_t row1, uint32_t nranks,
                     std::vector<uint32_t>& ord) {
    const uint32_t groups = groups_x * groups_y;
    std::vector<uint8_t> own_g(groups);
    for (uint32_t g = 0; g < groups; ++g) {
        const uint32_t gy = g / groups_x;
        own_g[g] = (nranks <= 1 || (row0 < row1 && gy * fg < row1 && (gy + 1) * fg > row0)) ? 1 : 0;
    }
    ord.clear();
    ord.reserve(groups);
    auto centre_d2 = [](float x, float y, float w, float h) {
        const float dx = x - 0.5f * w, dy = y - 0.5f * h;
        return dx * dx + dy * dy;
    };
    // super-groups by the distance of their centre (clipped to the grid) from the grid's
    const uint32_t sx_n = (groups_x + kSG - 1) / kSG, sy_n = (groups_y + kSG - 1) / kSG;
    std::vector<uint32_t> sgs(sx_n * sy_n);
    std::vector<float> d2(sgs.size());
    for (uint32_t k = 0; k < sgs.size(); ++k) {
        sgs[k] = k;
        const float cx = std::min((float)((k % sx_n) * kSG) + 0.5f * kSG, (float)groups_x);
        const float cy = std::min((float)((k / sx_n) * kSG) + 0.5f * kSG, (float)groups_y);
        d2[k] = centre_d2(cx, cy, (float)groups_x, (float)groups_y);
    }
    std::stable_sort(sgs.begin(), sgs.end(), [&](uint32_t a, uint32_t c) { return d2[a] < d2[c]; });
    // super-groups with a group of this rank's, dealt round-robin over the XCDs
    std::vector<std::vector<uint32_t>> xl(kXcds);
    uint32_t dealt = 0, total = 0;
    for (uint32_t j = 0; j < sgs.size(); ++j) {
        const uint32_t sx = sgs[j] % sx_n, sy = sgs[j] / sx_n;
        std::vector<uint32_t>& l = xl[dealt % kXcds];
        const size_t before = l.size();
        for (uint32_t gy = sy * kSG; gy < std::min((sy + 1) * kSG, groups_y); ++gy)
            for (uint32_t gx = sx * kSG; gx < std::min((sx + 1) * kSG, groups_x); ++gx)
                if (own_g[gy * groups_x + gx]) l.push_back(gy * groups_x + gx);
        if (l.size() > before) {
            total += (uint32_t)(l.size() - before);
            ++dealt;
        }
    }
    // workgroup i takes the next group of XCD i % kXcds's list (or of the longest list left)
    std::vector<size_t> pos(kXcds, 0);
    for (uint32_t i = 0; i < total; ++i) {
        uint32_t x = i % kXcds;
        if (pos[x] == xl[x].size()) {
            size_t best = 0;
            for (uint32_t y = 0; y < kXcds; ++y)
                if (xl[y].size() - pos[y] > best) { best = xl[y].size() - pos[y]; x = y; }
        }
        ord.push_back(xl[x][pos[x]++]);
    }
    for (uint32_t g = 0; g < groups; ++g)
        if (!own_g[g]) ord.push_back(g);
    return total;
}

// Centre-out order of a rank share's R render units (kDeal local tiles each) of the band [row0, row1): by the distance
// of a unit's middle tile from the band's centre (the central units cost the most; started first, the launch ends on
// the light border units): 8-rank C3 share 0.308 -> 0.292 ms (r03, round-robin deal)
void unit_order_centre(uint32_t R, uint32_t row0, uint32_t row1, uint32_t tiles_x, uint32_t* perm) {
    std::vector<float> d2(R);
    const float cy = 0.5f * (float)(row0 + row1);
    for (uint32_t q = 0; q < R; ++q) {
        uint32_t tx, ty;
        band_tile(q * kDeal + kDeal / 2, row0, row1, tiles_x, tx, ty);
        const float dx = ((float)tx + 0.5f) - 0.5f * (float)tiles_x, dy = ((float)ty + 0.5f) - cy;
        d2[q] = dx * dx + dy * dy;
        perm[q] = q;
    }
    std::stable_sort(perm, perm + R, [&](uint32_t a, uint32_t c) { return d2[a] < d2[c]; });
}

// The R units' costs from a whole frame's tile costs (tile_cost: the frame's tiles_x x tiles_y tiles in its own local
// order, k_render_cor's tile_cost of a one-rank frame)
void unit_costs(const uint32_t* tile_cost, uint32_t R, uint32_t row0, uint32_t row1, uint32_t tiles_x, uint32_t tiles_y,
                double* cost) {
    for (uint32_t q = 0; q < R; ++q) {
        cost[q] = 0.0;
        for (uint32_t i = 0; i < kDeal; ++i) {
            uint32_t tx, ty;
            band_tile(q * kDeal + i, row0, row1, tiles_x, tx, ty);
            cost[q] += tile_cost[band_index(tx, ty, 0, tiles_y, tiles_x)];
        }
    }
}

// The deal of a rank share's R render units (R a multiple of kXcds) over the XCDs: by cost, longest first (ties in the
// centre-out order), each unit to the XCD with the least cost so far among those holding fewer than R / kXcds; perm
// position k kXcds + x holds XCD x's k-th unit (xcd_local_tile_perm), so each XCD starts its longest units first
void deal_units(const double* cost, const uint32_t* centre, uint32_t R, uint32_t* perm) {
    std::vector<uint32_t> by(centre, centre + R);
    std::stable_sort(by.begin(), by.end(), [&](uint32_t a, uint32_t c) { return cost[a] > cost[c]; });
    double load[kXcds] = {};
    uint32_t count[kXcds] = {};
    for (uint32_t q : by) {
        uint32_t x = kXcds;
        for (uint32_t j = 0; j < kXcds; ++j)
            if (count[j] < R / kXcds && (x == kXcds || load[j] < load[x])) x = j;
        perm[count[x] * kXcds + x] = q;
        load[x] += cost[q];
        ++count[x];
    }
}

// The refusals of a whole frame. Each flag of kFrameFlags in the mode is checked on its own, the gradient flags first and
// newest first, then the two second outputs oldest first: its entry point, COR, not the counting pass, not dump codes, not
// the LUT where its row says so, none of the flags before it in the table, and for a gradient frame no mesh. The first refusal wins; then the checks every frame
// gets.
Refusal frame_refusal(uint32_t mode, GradKind caller, uint32_t samples, const SceneFacts& sc) {
    constexpr int N = (int)(sizeof kFrameFlags / sizeof kFrameFlags[0]);
    const uint32_t low = mode & 0xffu;
    auto why_not = [&](int i, bool grad) -> std::string {  // flag i of the table, if the mode has it and it is of that sort
        const FrameFlag& F = kFrameFlags[i];
        if (!(mode & F.bit) || (F.kind != GradKind::none) != grad) return "";
        const std::string name = std::string(F.name) + ": ";
        if (grad && caller != F.kind) return name + "only through " + F.entry + " (the gradient image goes there)";
        if (low != GSRT_MODE_COR) return name + "COR frames only";
        if (mode & GSRT_FLAG_STATS) return name + "not with GSRT_FLAG_STATS";
        if (mode & GSRT_FLAG_OUT_DUMP8) return name + "not with GSRT_FLAG_OUT_DUMP8";
        if (F.no_lut && (mode & GSRT_FLAG_LUT)) return name + "not with GSRT_FLAG_LUT";
        for (int j = 0; j < i; ++j)
            if (mode & kFrameFlags[j].bit) return name + "not with " + kFrameFlags[j].name;
        return grad && sc.ntri ? name + "not for a scene with a triangle mesh" : "";
    };
    std::string why;
    for (int i = N - 1; i >= 0 && why.empty(); --i) why = why_not(i, true);
    for (int i = 0; i < N && why.empty(); ++i) why = why_not(i, false);
    if (!why.empty()) return {GSRT_E_ARG, why};
    if (low > GSRT_MODE_COR || (mode & ~(0xffu | GSRT_FLAG_LUT | GSRT_FLAG_STATS | frame_flag_bits()))) return {GSRT_E_ARG, "bad mode"};
    if (low == GSRT_MODE_COR && samples == 0) return {GSRT_E_ARG, "samples == 0"};
    if (!sc.bvh_built) return {GSRT_E_STATE, "render before gsrt_build_bvh"};
    if (sc.ntri && low != GSRT_MODE_REF) return {GSRT_E_ARG, "triangle meshes are co-traced in REF mode only"};
    if ((mode & GSRT_FLAG_FEATURES) && !sc.features)
        return {GSRT_E_STATE, "GSRT_FLAG_FEATURES: the scene has no feature table (gsrt_scene_set_features)"};
    for (const FrameFlag& F : kFrameFlags)
        if ((mode & F.bit) && F.needs_sh && !sc.sh)
            return {GSRT_E_STATE, std::string(F.name) + ": the scene has no SH rows (gsrt_scene_set_sh)"};
    return {GSRT_OK, ""};
}

}  // namespace gsrt

extern "C" gsrt_status gsrt_debug_frame_refusal_any(uint32_t mode, uint32_t caller, uint32_t samples, int bvh_built,
                                                    uint32_t ntri, int has_features, int has_sh, char* msg, size_t cap) {
    if (caller > (uint32_t)gsrt::GradKind::splat_depth) return GSRT_E_ARG;
    const gsrt::Refusal r = gsrt::frame_refusal(mode, (gsrt::GradKind)caller, samples,
                                                {bvh_built != 0, ntri, has_features != 0, has_sh != 0});
    if (msg && cap) {
        const size_t len = std::min(r.msg.size(), cap - 1);
        std::memcpy(msg, r.msg.data(), len);
        msg[len] = '\0';
    }
    return r.status;
}

// the hook as it was before the callers past gsrt_render_splat_grad: those it refuses
extern "C" gsrt_status gsrt_debug_frame_refusal_kind(uint32_t mode, uint32_t caller, uint32_t samples, int bvh_built,
                                                     uint32_t ntri, int has_features, int has_sh, char* msg, size_t cap) {
    if (caller > (uint32_t)gsrt::GradKind::splat) return GSRT_E_ARG;
    return gsrt_debug_frame_refusal_any(mode, caller, samples, bvh_built, ntri, has_features, has_sh, msg, cap);
}

// the hook as it was before the callers past gsrt_render_opacity_grad: those it refuses
extern "C" gsrt_status gsrt_debug_frame_refusal(uint32_t mode, uint32_t caller, uint32_t samples, int bvh_built, uint32_t ntri,
                                                int has_features, int has_sh, char* msg, size_t cap) {
    if (caller > (uint32_t)gsrt::GradKind::opacity) return GSRT_E_ARG;
    return gsrt_debug_frame_refusal_kind(mode, caller, samples, bvh_built, ntri, has_features, has_sh, msg, cap);
}

extern "C" gsrt_status gsrt_deal_units(const double* cost, const uint32_t* centre, uint32_t units, uint32_t* perm) {
    if (!cost || !centre || !perm || units % gsrt::kXcds) return GSRT_E_ARG;
    std::vector<uint8_t> seen(units, 0);  // centre must be a permutation of the units
    for (uint32_t i = 0; i < units; ++i) {
        if (centre[i] >= units || seen[centre[i]]) return GSRT_E_ARG;
        seen[centre[i]] = 1;
    }
    gsrt::deal_units(cost, centre, units, perm);
    return GSRT_OK;
}

extern "C" gsrt_status gsrt_group_order(uint32_t groups_x, uint32_t groups_y, uint32_t fg, uint32_t row0, uint32_t row1,
                                        uint32_t nranks, uint32_t* ord, uint32_t* own) {
    if (!ord || !own || groups_x == 0 || groups_y == 0 || fg == 0 || row0 > row1) return GSRT_E_ARG;
    if ((uint64_t)groups_x * groups_y > 0xffffffffull) return GSRT_E_ARG;
    std::vector<uint32_t> o;
    *own = gsrt::group_order(groups_x, groups_y, fg, row0, row1, nranks, o);
    std::copy(o.begin(), o.end(), ord);
    return GSRT_OK;
}

extern "C" gsrt_status gsrt_unit_order(uint32_t units, uint32_t row0, uint32_t row1, uint32_t tiles_x, uint32_t* perm) {
    if (!perm || units % gsrt::kXcds || tiles_x == 0 || row0 >= row1) return GSRT_E_ARG;
    // the units are whole within the band's tiles (launch_render: R = the band's complete XCD rounds)
    if ((uint64_t)units * gsrt::kDeal > (uint64_t)tiles_x * (row1 - row0)) return GSRT_E_ARG;
    gsrt::unit_order_centre(units, row0, row1, tiles_x, perm);
    return GSRT_OK;
}
