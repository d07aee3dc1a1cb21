"""An independent float64 restatement of the COR render ("COR flags") -- test infrastructure.

It shares no code and no operation order with oracle/gsrt_oracle.c or the HIP kernels: every quantity is computed
in float64 with numpy's own formulas, the exponential is np.exp, candidates are found by brute force over all
Gaussians, and the blend walks each ray's hits in (depth, id) order. The structure it follows is the reference's:
  - Gaussian covariance and AABB: Gauss::init_cov3d / init_radius (RayTracingInVulkan/src/Assets/Sphere.hpp:129-165);
  - primary rays with the pixel jitter of RayTracing.rgen:27-43 (RandomFloat / RandomInt, Random.glsl:24-37;
    every pixel starts from Camera.RandomSeed);
  - candidate set: the exact AABB slab test on [0.001, 10000] (vulkan_ray_tracing.cc:217-237);
  - per candidate, the EWA projection of RayTracing.ProceduralGauss.rint:62-102 with the COR flags: depth = -view z,
    the true Jacobian (fx = P00 W/2, fy = P11 H/2), V + 0.3 I, conic = (V + 0.3 I)^-1, g = 1/2 d^T conic d,
    0 <= g <= 5.6, alpha = min(opacity exp(-g), 0.99), kept when alpha > 1/255;
  - front-to-back blend (rchit:15-33 with the COR flags): C += T alpha colour, T *= 1 - alpha, stop before a hit
    that would take T below 1e-4; colour = max(0, 0.5 + sum_k sh_k Y_k(dir)) (3DGS SH-3 basis) or 1 without SH;
    output (C, 1 - T) averaged over the samples.

Decisions that float32 rounding can flip are reported per pixel and those pixels are excluded from the comparison
(SURVEY.md §8c): an alpha within `alpha_rel` of 1/255, a T(1 - alpha) within `trans_rel` of 1e-4, a slab test
within `slab_rel` of its boundary, two contributing hits of different colour whose depths differ by less than
`depth_rel` (their float32 order can swap), and a projection whose determinant is within `det_rel` of zero. Two more
are reported for the sake of the gradients, which jump where the frame is only kinked: a blended hit whose o e is within
`alpha_rel` of 0.99, and one with a channel whose colour before the clamp at 0 is within `col_rel` of 0, relative to the
size of the terms it sums.

gradients() is the backward of the same blend to the opacities, the SH table and a feature table, derived from the
definition above (its docstring) and not from the kernels' two-sweep form; it walks the hit lists render walks.
"""
import hashlib

import numpy as np

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)


def covariance(rot, scale):
    """Sigma = (S R)^T (S R) with R the glm::mat3 Sphere.hpp:143-147 builds from (r, x, y, z), in float64."""
    q = np.asarray(rot, np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    # glm's mat3 constructor is column-major: argument k lands in column k // 3, row k % 3
    cols = np.stack([
        np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)], -1),
        np.stack([2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)], -1),
        np.stack([2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1)], -1)  # [n, row, col]
    M = np.asarray(scale, np.float64)[:, :, None] * cols  # S * R: row i of R scaled by s_i
    return np.einsum("nki,nkj->nij", M, M)


def _mat(a):
    return np.asarray(a, np.float64).reshape(4, 4).T  # column-major storage -> math matrix


class Ubo:
    def __init__(self, ubo):
        u = ubo.reshape(-1)[0] if ubo.dtype.names else ubo
        self.MV = _mat(u["model_view"])
        self.P = _mat(u["projection"])
        self.MVi = _mat(u["model_view_inverse"])
        self.Pi = _mat(u["projection_inverse"])
        self.W, self.H = int(u["width"]), int(u["height"])
        self.S = max(1, int(u["samples"]))
        self.seed = int(u["random_seed"])
        self.focus = float(u["focus_distance"])


def jitter(seed, samples):
    """RandomFloat pairs from the LCG, x first then y (RayTracing.rgen:38)."""
    out = []
    s = seed & 0xFFFFFFFF
    for _ in range(samples):
        pair = []
        for _ in range(2):
            s = (1664525 * s + 1013904223) & 0xFFFFFFFF
            pair.append((s & 0xFFFFFF) / float(1 << 24))
        out.append(pair)
    return out


def rays(u, px, py):
    """origin (3,) and unit directions (n, 3) for pixel coordinates px, py (float64 arrays)."""
    uv = np.stack([px / u.W * 2.0 - 1.0, py / u.H * 2.0 - 1.0, np.ones_like(px), np.ones_like(px)], -1)
    tg = uv @ u.Pi.T
    v = tg[:, :3] * u.focus
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    d = v @ u.MVi[:3, :3].T
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    o = u.MVi[:3, 3]
    return o, d


def sh_basis(d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz = x * x, y * y, z * z
    return np.stack([
        np.full_like(x, SH_C0), -SH_C1 * y, SH_C1 * z, -SH_C1 * x,
        SH_C2[0] * x * y, SH_C2[1] * y * z, SH_C2[2] * (2 * zz - xx - yy), SH_C2[3] * x * z, SH_C2[4] * (xx - yy),
        SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * x * y * z, SH_C3[2] * y * (4 * zz - xx - yy),
        SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
        SH_C3[6] * x * (xx - 3 * yy)], -1)


class Splats:
    """Per-Gaussian screen-space quantities (the rint projection with the COR flags), float64."""

    def __init__(self, u, center, rot, scale, opacity, sh=None, det_rel=1e-6):
        c = np.asarray(center, np.float64)
        n = len(c)
        self.n = n
        rad = 3.0 * np.asarray(scale, np.float64).max(1)
        self.lo, self.hi = c - rad[:, None], c + rad[:, None]
        t = np.concatenate([c, np.ones((n, 1))], 1) @ u.MV.T
        self.depth = -t[:, 2]
        ph = t @ u.P.T
        self.ppx = (ph[:, 0] / ph[:, 3] + 1.0) * u.W / 2.0
        self.ppy = (ph[:, 1] / ph[:, 3] + 1.0) * u.H / 2.0
        fx, fy = u.P[0, 0] * u.W / 2.0, u.P[1, 1] * u.H / 2.0
        dd = np.where(self.depth > 0, self.depth, 1.0)
        J = np.zeros((n, 2, 3))
        J[:, 0, 0] = fx / dd
        J[:, 0, 2] = fx * t[:, 0] / dd ** 2
        J[:, 1, 1] = fy / dd
        J[:, 1, 2] = fy * t[:, 1] / dd ** 2
        T = J @ u.MV[:3, :3]
        V = T @ covariance(rot, scale) @ np.transpose(T, (0, 2, 1)) + 0.3 * np.eye(2)
        det = V[:, 0, 0] * V[:, 1, 1] - V[:, 0, 1] * V[:, 1, 0]
        self.valid = (self.depth > 0) & (det > 0)
        self.det_near = np.abs(det) <= det_rel * np.abs(V[:, 0, 0] * V[:, 1, 1])
        sd = np.where(self.valid, det, 1.0)
        self.ca, self.cb, self.cc = V[:, 1, 1] / sd, -V[:, 0, 1] / sd, V[:, 0, 0] / sd
        self.opacity = np.asarray(opacity, np.float64)
        self.sh = None if sh is None else np.asarray(sh, np.float64).reshape(n, 16, 3)


class _Subset:
    """the AABBs of some Gaussians (what _tile_candidates reads)"""

    def __init__(self, sp, idx):
        self.lo, self.hi, self.n = sp.lo[idx], sp.hi[idx], len(idx)


def _tile_candidates(u, sp, x0, x1, y0, y1):
    """Gaussians whose bounding sphere (centre, sqrt(3) x radius) meets the pyramid of all rays through the pixel
    rectangle [x0, x1] x [y0, y1]: a necessary condition for any of those rays to hit the AABB (the pyramid's side
    planes contain the origin and two corner directions; directions are a projective map of the screen point)."""
    cx = np.array([x0, x1, x1, x0], np.float64)
    cy = np.array([y0, y0, y1, y1], np.float64)
    o, d = rays(u, cx, cy)
    inner = d.mean(0)
    c = (sp.lo + sp.hi) * 0.5 - o
    rad = np.linalg.norm(sp.hi - sp.lo, axis=1) * 0.5 * (1.0 + 1e-9) + 1e-9
    keep = np.ones(sp.n, bool)
    for k in range(4):
        n = np.cross(d[k], d[(k + 1) % 4])
        n /= np.linalg.norm(n)
        if n @ inner < 0:
            n = -n
        keep &= c @ n >= -rad
    return np.nonzero(keep)[0]


THR_A = 1.0 / 255.0


def _tiles(u, sp, r0, r1, tile):
    """the frame's tiles: (ty, ye, tx, xe), the tile's candidate Gaussians and its pixels' integer coordinates (float64)"""
    # the band's pyramid first (every tile's pyramid lies inside it), then each tile's among those
    band = _tile_candidates(u, sp, 0, u.W, r0, r1)
    sub = _Subset(sp, band)
    for ty in range(r0, r1, tile):
        for tx in range(0, u.W, tile):
            ye, xe = min(ty + tile, r1), min(tx + tile, u.W)
            cand = band[_tile_candidates(u, sub, tx, xe, ty, ye)]
            ys, xs = np.mgrid[ty:ye, tx:xe]
            yield (ty, ye, tx, xe), cand, xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64)


def render(ubo, center, rot, scale, opacity, sh=None, rows=None, tile=16, alpha_rel=1e-3, trans_rel=1e-3,
           slab_rel=1e-5, depth_rel=1e-6, col_rel=1e-4):
    """RGBA (H, W, 4) float64 and a bool (H, W) mask of pixels with a decision near a threshold."""
    u = Ubo(ubo)
    sp = Splats(u, center, rot, scale, opacity, sh)
    r0, r1 = rows if rows else (0, u.H)
    out = np.zeros((u.H, u.W, 4))
    near = np.zeros((u.H, u.W), bool)
    jit = jitter(u.seed, u.S)
    for (ty, ye, tx, xe), cand, xs, ys in _tiles(u, sp, r0, r1, tile):
        m = len(xs)
        acc = np.zeros((m, 4))
        tile_near = np.zeros(m, bool)
        for jx, jy in jit:
            px, py = xs + jx, ys + jy
            o, d = rays(u, px, py)
            C = np.zeros((m, 3))
            T = np.ones(m)
            if len(cand):
                hits = _hits(sp, cand, px, py, o, d, tile_near, alpha_rel, slab_rel, depth_rel)
                C, T = _walk(hits, m, tile_near, trans_rel)[:2]
                _clamps_near(sp, hits, tile_near, alpha_rel, col_rel)
            acc[:, :3] += C
            acc[:, 3] += 1.0 - T
        out[ty:ye, tx:xe] = acc.reshape(ye - ty, xe - tx, 4)
        near[ty:ye, tx:xe] = tile_near.reshape(ye - ty, xe - tx)
    return out[r0:r1] / u.S, near[r0:r1]


class _Hits:
    """One sample's hit lists, every ray's hits in (depth, id) order, rays ascending: ri the ray, gi the Gaussian,
    alpha = min(o e, 0.99), oe = o e before that clamp, e = exp(-g), col = max(0, pre), pre the SH colour before its
    clamp at 0 (None without SH rows) and Y the ray's SH basis (likewise). _walk adds, per hit, `blended` (the blend took
    it: the ray had not stopped) and `T` (the transmittance before it)."""


def _hits(sp, cand, px, py, o, d, ray_near, alpha_rel, slab_rel, depth_rel):
    """Selection and ordering, shared by render and gradients; marks ray_near for the decisions taken here."""
    thr_a = THR_A
    lo, hi = sp.lo[cand], sp.hi[cand]
    # exact slab test on [0.001, 10000], every ray against every candidate box
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        t0 = (lo[None, :, :] - o) * inv[:, None, :]
        t1 = (hi[None, :, :] - o) * inv[:, None, :]
    tn = np.maximum(np.nanmax(np.minimum(t0, t1), axis=2), 0.001)
    tf = np.minimum(np.nanmin(np.maximum(t0, t1), axis=2), 10000.0)
    hit = tn <= tf
    amb = np.abs(tf - tn) <= slab_rel * np.maximum(1.0, np.abs(tn))
    ri, ci = np.nonzero((hit | amb) & sp.valid[cand][None, :])
    gi = cand[ci]
    dx, dy = px[ri] - sp.ppx[gi], py[ri] - sp.ppy[gi]
    g = 0.5 * (sp.ca[gi] * dx * dx + 2.0 * sp.cb[gi] * dx * dy + sp.cc[gi] * dy * dy)
    e = np.exp(-g)
    oe = sp.opacity[gi] * e
    alpha = np.minimum(oe, 0.99)
    keep = (g >= 0.0) & (g <= 5.6) & (alpha > thr_a)
    # decisions float32 may take the other way: a box grazed by a contributing splat's ray, alpha at 1/255,
    # a projection whose determinant is ~0
    a_near = np.abs(alpha / thr_a - 1.0) <= alpha_rel
    pair_amb = (amb[ri, ci] & (alpha > thr_a * (1 - alpha_rel))) | a_near | sp.det_near[gi]
    np.logical_or.at(ray_near, ri[pair_amb], True)
    sel = keep & hit[ri, ci]
    ri, gi, alpha, oe, e = ri[sel], gi[sel], alpha[sel], oe[sel], e[sel]
    order = np.lexsort((gi, sp.depth[gi], ri))  # per ray, (depth, id) order
    ri, gi, alpha, oe, e = ri[order], gi[order], alpha[order], oe[order], e[order]
    depth = sp.depth[gi]
    pre = Y = None
    if sp.sh is not None:
        Y = sh_basis(d)[ri]
        pre = 0.5 + np.einsum("pk,pkc->pc", Y, sp.sh[gi])
        col = np.maximum(0.0, pre)
    else:
        col = np.ones((len(ri), 3))
    # two hits whose float32 depths may compare the other way: swapping them moves the pixel by at most
    # T a1 a2 |c1 - c2| (the blend of equal colours is order-independent), so only a visible swap is ambiguous
    same = (ri[1:] == ri[:-1]) & (np.abs(depth[1:] - depth[:-1]) <= depth_rel * depth[1:])
    swing = alpha[1:] * alpha[:-1] * np.abs(col[1:] - col[:-1]).max(1)
    np.logical_or.at(ray_near, ri[1:][same & (swing > 1e-4)], True)
    h = _Hits()
    h.ri, h.gi, h.alpha, h.oe, h.e, h.col, h.pre, h.Y = ri, gi, alpha, oe, e, col, pre, Y
    return h


def _walk(h, m, ray_near, trans_rel):
    """Front to back over the hit lists of m rays: C (m, 3), T (m,) and the rays a stop ended (m,) bool; sets h.blended
    and h.T. A ray stops before the first hit that would take T below 1e-4 and blends nothing behind it."""
    ri, alpha, col = h.ri, h.alpha, h.col
    # the k-th hit of every ray at once
    starts = np.searchsorted(ri, np.arange(m))
    counts = np.bincount(ri, minlength=m)
    T = np.ones(m)
    C = np.zeros((m, 3))
    live = np.ones(m, bool)
    h.blended = np.zeros(len(ri), bool)
    h.T = np.zeros(len(ri))
    for k in range(int(counts.max()) if len(ri) else 0):
        rr = np.nonzero(live & (counts > k))[0]
        if not len(rr):
            break
        p = starts[rr] + k
        tnext = T[rr] * (1.0 - alpha[p])
        ray_near[rr[np.abs(tnext / 1e-4 - 1.0) <= trans_rel]] = True
        stop = tnext < 1e-4
        live[rr[stop]] = False
        go, pg = rr[~stop], p[~stop]
        h.blended[pg] = True
        h.T[pg] = T[go]
        C[go] += (T[go] * alpha[pg])[:, None] * col[pg]
        T[go] = tnext[~stop]
    return C, T, ~live


def _clamps_near(sp, h, ray_near, alpha_rel, col_rel):
    """The two clamps of a blended hit that float32 may take the other way. The frame is continuous across both; the
    opacity gradient jumps at o e = 0.99 and the SH gradient at pre = 0. A channel's pre is a sum of 17 terms, so its
    float32 error scales with 0.5 + sum_q |s_q Y_q|, not with pre."""
    b = h.blended
    ray_near[h.ri[b][np.abs(h.oe[b] / 0.99 - 1.0) <= alpha_rel]] = True
    if h.pre is not None:
        mag = 0.5 + np.einsum("pk,pkc->pc", np.abs(h.Y[b]), np.abs(sp.sh[h.gi[b]]))
        ray_near[h.ri[b][(np.abs(h.pre[b]) <= col_rel * mag).any(1)]] = True


def _scatter(out, idx, val):
    """out[idx[k]] += val[k] with repeated indices, each row of out summed in the order of k"""
    if not len(idx):
        return
    order = np.argsort(idx, kind="stable")
    s = idx[order]
    first = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    out[s[first]] += np.add.reduceat(val[order], first, axis=0)


class Gradients:
    """What gradients() returns: opacity (n,), sh (n, 16, 3) or None, feat (n, C) or None; M_opacity, M_sh, M_feat, the
    sum of the absolute values of the terms each entry sums; near (rows, W) bool; digest, a hash of the hit lists (ray,
    Gaussian, whether o e < 0.99); gauss_clamped, gauss_open (n,) bool: the Gaussian has a clamped / an open hit; counts, a dict of events over the frame's sample rays (mean_alpha: the mean of the
    frame's alpha channel)."""


def gradients(ubo, center, rot, scale, opacity, sh=None, *, G_rgba=None, G_feat=None, rows=None, tile=16,
              alpha_rel=1e-3, trans_rel=1e-3, slab_rel=1e-5, depth_rel=1e-6, col_rel=1e-4, clamp_selects=True):
    """The backward of render, from the blend's definition (module docstring), in float64. L = <G_rgba, rgba> for the
    opacities and the SH table, L = <G_feat, feat> for a feature table (feat_c = sum_i f[g_i, c] w_i / ns, which is
    linear in f). G_rgba is (H, W, 4), G_feat (H, W, C); with rows, only those rows are read.
    For a ray with blended hits i = 1..N in (depth, id) order, alpha_i = min(o e_i, 0.99), T_i = prod_{j<i} (1 - alpha_j),
    w_i = alpha_i T_i, col_i = max(0, pre_i), Gs = G / ns:
        rgb = sum_i col_i w_i, a = 1 - T_{N+1}
        d rgb / d alpha_i = T_i col_i - S_i / (1 - alpha_i), S_i = sum_{j>i} col_j w_j (every later w_j carries the
                            factor 1 - alpha_i), and d a / d alpha_i = T_{N+1} / (1 - alpha_i);
        dL/d alpha_i = sum_ch Gs_ch (T_i col_{i,ch} - S_{i,ch} / (1 - alpha_i)) + Gs_3 T_{N+1} / (1 - alpha_i)
        grad_o[g_i] += dL/d alpha_i e_i           where o e_i < 0.99 (else alpha_i is the constant 0.99)
        grad_sh[g_i, q, ch] += w_i Y_q Gs_ch      where pre_{i,ch} > 0 (else col is the constant 0)
        grad_feat[g_i, c] += w_i G_feat[p, c] / ns
    S_i is summed from the ray's last hit backwards, never as a difference of two sums. The hits, their order, the 1/255
    and g <= 5.6 cuts and the stop are the forward's and are not differentiated. The magnitudes M sum the absolute value
    of every product above: |Gs_ch| T_i col e, |Gs_ch| S_i / (1 - alpha_i) e and |Gs_3| T_{N+1} / (1 - alpha_i) e for an
    opacity, |w Y_q Gs_ch| for an SH coefficient, |w G_feat / ns| for a feature.
    clamp_selects=False leaves both `where`s out (a backward that forgot the clamps), for tests of the tests' power."""
    u = Ubo(ubo)
    sp = Splats(u, center, rot, scale, opacity, sh)
    n = sp.n
    r0, r1 = rows if rows else (0, u.H)
    near = np.zeros((u.H, u.W), bool)
    jit = jitter(u.seed, u.S)
    out = Gradients()
    Gr = None if G_rgba is None else np.asarray(G_rgba, np.float64).reshape(u.H, u.W, 4) / u.S
    Gf = None if G_feat is None else np.asarray(G_feat, np.float64).reshape(u.H, u.W, -1) / u.S
    out.opacity, out.M_opacity = np.zeros(n), np.zeros(n)
    out.sh = out.M_sh = out.feat = out.M_feat = None
    if sp.sh is not None and Gr is not None:
        out.sh, out.M_sh = np.zeros((n, 16, 3)), np.zeros((n, 16, 3))
    if Gf is not None:
        out.feat, out.M_feat = np.zeros((n, Gf.shape[2])), np.zeros((n, Gf.shape[2]))
    cnt = dict(hits=0, clamped=0, clamped_behind=0, stopped_rays=0, channels=0, channels_clamped=0, alpha_sum=0.0)
    g_clamped, g_open = np.zeros(n, bool), np.zeros(n, bool)
    pair_clamped, pair_open = np.zeros((n, 3), bool), np.zeros((n, 3), bool)
    digest = hashlib.sha256()
    for (ty, ye, tx, xe), cand, xs, ys in _tiles(u, sp, r0, r1, tile):
        m = len(xs)
        tile_near = np.zeros(m, bool)
        iy, ix = ys.astype(np.int64), xs.astype(np.int64)
        for s, (jx, jy) in enumerate(jit):
            if not len(cand):
                continue
            px, py = xs + jx, ys + jy
            o, d = rays(u, px, py)
            h = _hits(sp, cand, px, py, o, d, tile_near, alpha_rel, slab_rel, depth_rel)
            _, T_end, stopped = _walk(h, m, tile_near, trans_rel)
            _clamps_near(sp, h, tile_near, alpha_rel, col_rel)
            b = h.blended  # a prefix of every ray's list
            r, g, a, Ti, col, e = h.ri[b], h.gi[b], h.alpha[b], h.T[b], h.col[b], h.e[b]
            is_open = h.oe[b] < 0.99
            w = a * Ti
            starts = np.searchsorted(r, np.arange(m))
            counts = np.bincount(r, minlength=m)
            pos = np.arange(len(r)) - starts[r]
            # the colour behind each hit, from the ray's last hit backwards
            S = np.zeros((len(r), 3))
            behind = np.zeros((m, 3))
            for k in range(int(counts.max()) - 1 if len(r) else -1, -1, -1):
                rr = np.nonzero(counts > k)[0]
                p = starts[rr] + k
                S[p] = behind[rr]
                behind[rr] += col[p] * w[p, None]
            digest.update(((iy[r] * u.W + ix[r]) * u.S + s).tobytes() + g.tobytes() + is_open.tobytes())
            cnt["hits"] += len(r)
            cnt["clamped"] += int((~is_open).sum())
            cnt["clamped_behind"] += int((~is_open & (pos > 0)).sum())
            cnt["stopped_rays"] += int(stopped.sum())
            cnt["alpha_sum"] += float((1.0 - T_end).sum())
            g_clamped[g[~is_open]] = True
            g_open[g[is_open]] = True
            on = np.ones((len(r), 3), bool)
            if h.pre is not None:
                on = h.pre[b] > 0.0
                cnt["channels"] += on.size
                cnt["channels_clamped"] += int((~on).sum())
                for ch in range(3):
                    pair_clamped[g[~on[:, ch]], ch] = True
                    pair_open[g[on[:, ch]], ch] = True
            if Gr is not None:
                Gs = Gr[iy[r], ix[r]]
                rinv = 1.0 / (1.0 - a)
                front, back = Ti[:, None] * col, S * rinv[:, None]
                tail = T_end[r] * rinv
                dLda = (Gs[:, :3] * (front - back)).sum(1) + Gs[:, 3] * tail
                mag = (np.abs(Gs[:, :3]) * (front + back)).sum(1) + np.abs(Gs[:, 3]) * tail
                use = is_open if clamp_selects else np.ones(len(r), bool)
                _scatter(out.opacity, g[use], (dLda * e)[use])
                _scatter(out.M_opacity, g[use], (mag * e)[use])
                if out.sh is not None:
                    wg = w[:, None] * Gs[:, :3]
                    if clamp_selects:
                        wg = np.where(on, wg, 0.0)
                    terms = h.Y[b][:, :, None] * wg[:, None, :]
                    _scatter(out.sh, g, terms)
                    _scatter(out.M_sh, g, np.abs(terms))
            if Gf is not None:
                terms = w[:, None] * Gf[iy[r], ix[r]]
                _scatter(out.feat, g, terms)
                _scatter(out.M_feat, g, np.abs(terms))
        near[ty:ye, tx:xe] = tile_near.reshape(ye - ty, xe - tx)
    cnt["gauss_clamped"], cnt["gauss_open"] = int(g_clamped.sum()), int(g_open.sum())
    cnt["mixed_pairs"] = int((pair_clamped & pair_open).sum())
    cnt["mean_alpha"] = cnt.pop("alpha_sum") / ((r1 - r0) * u.W * u.S)  # the frame's mean alpha, 1 - T
    out.near, out.counts, out.digest = near[r0:r1], cnt, digest.hexdigest()
    out.gauss_clamped, out.gauss_open = g_clamped, g_open
    return out
