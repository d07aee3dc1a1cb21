"""Constructed scenes whose tiles hold more candidates than their first list (kCap = 256 ids), with their cameras, float64
references and planted faults: shared by tests/test_deep_grad_ref.py (CPU: the conditions every scene must meet and the
comparison's power) and tests/test_deep_grad_gpu.py (every gradient and forward kind held to float64 on them).

A random deep cloud is useless here: nearly every pixel of one is float32-sensitive (cor_f64's `near`) and the upstream
gradient would be zero almost everywhere. The scenes are built so that a ray of several hundred to two thousand hits takes
no decision float32 can take the other way, under the origin camera at fovy 20 (view depth = -z exactly):
  - faint: Gaussians wider than the frame (scale 1.2..1.5 z, centres within 0.05 z of the axis), opacity just above 1/255:
    alpha lies in a band 5 % and more above the cut on every ray, so every one of them is a hit of every ray and a candidate
    of every tile and group, and T falls by under 0.5 % per hit. Their number decides the path a case takes;
  - opaque: the same shape behind them (opacity 0.5..0.7): the faint layer ends with T well above 1e-4, and the crossing of
    1e-4, the stop, takes large steps here, so few rays land in the `trans_rel` band;
  - small: a few pixels wide, scattered over the frame among the faint ones: they make the tiles' lists differ, so that the
    tile filter and every tile's own resume position in its group's list matter;
  - clamped: opacity 1, about a pixel wide, centred on the first sample of chosen pixels in the middle of the faint layer:
    alpha is clamped at 0.99 behind other hits;
  - pins (`passes` only): opacity 0.0055, centred on the second sample of chosen pixels: a few dozen hits each, within
    half a pixel of that sample, so that one sample's terms are a visible share of their table entries (a pass counted
    twice shows on them);
  - SH rows: coefficient 0 puts every colour channel before its clamp at 0 in 0.3..1.2 or in -0.8..-0.3, the other 15
    coefficients lie within 0.01: both states of the clamp occur and no channel is near 0.
Depths are distinct by construction (a permutation of slots, a jitter inside each).

A case is (name, width, height, spp); the path it takes in k_render_cor, by the counts test_deep_grad_ref.py asserts:
  cut       every tile's list is cut at 256, the group's first segment (896 keys) holds the group: the rounds after the
            first resume at the tile's position in the group's list. 1 spp (8x8-pixel tiles) and 4 spp (4x4);
  segment   more than 896 and fewer than 1792 per group at 16 spp: launch_render runs k_group_more, which writes the
            second segment, only where a tile holds at least 16 samples per pixel (kMoreLanes); 2x2-pixel tiles;
  traverse  more than 1792 per tile at 1 spp: k_group_more does not run, so past the first segment's 896 keys every tile
            traverses on its own in rounds of 128;
  passes    80 and 130 spp, one pixel per lane, the sweeps run once per pass; more than 256 per tile.
"""
import contextlib
import math

import numpy as np

import cor_f64 as F
import cor_f64_depth as D
import cor_f64_geom as Q
import oracle as O

FOVY = 20.0
K_CAP, K_GCAP, K_GLIST = 256, 896, 1792  # ids of a tile's list, keys of a group-list segment, of a group's whole list
MV = O.lookat((0, 0, 0), (0, 0, -1))
CASES = [("cut", 24, 16, 1), ("cut", 24, 16, 4), ("segment", 10, 7, 16), ("traverse", 24, 16, 1), ("passes", 12, 10, 80),
         ("passes", 12, 10, 130)]
# per scene: the frame it is built for, the layers' sizes, the faint opacities, the small ones' sigma in pixels and opacity
SCENES = {
    "cut": dict(frame=(24, 16), faint=420, opaque=60, small=150, clamped=6, faint_o=(0.0045, 0.0048), small_px=(1.0, 3.0),
                small_o=(0.05, 0.3), seed=401),
    "segment": dict(frame=(10, 7), faint=1000, opaque=100, small=40, clamped=4, faint_o=(0.0045, 0.0048),
                    small_px=(0.5, 1.0), small_o=(0.05, 0.3), seed=402),
    "traverse": dict(frame=(24, 16), faint=1650, opaque=200, small=300, clamped=6, faint_o=(0.0044, 0.0046),
                     small_px=(0.7, 2.0), small_o=(0.02, 0.08), seed=403),
    "passes": dict(frame=(12, 10), faint=270, opaque=40, small=12, clamped=3, faint_o=(0.0045, 0.0048),
                   small_px=(0.4, 0.8), small_o=(0.05, 0.3), pins=8, seed=404),
}
_CACHE = {}


def case_id(case):
    return "%s-%dx%d-spp%d" % case


def camera(case):
    _, w, h, spp = case
    return O.make_ubo(MV, FOVY, w, h, 1.0, spp, 16)


def kernel_tile(spp):
    """(tile width, tile height, samples per pixel in the wave) of a COR frame: make_plan in gsrt_plan.cpp. Frames this
    small take groups of 2x2 tiles."""
    if spp <= 64 and spp & (spp - 1) == 0:
        lg = (64 // spp).bit_length() - 1
        return 1 << ((lg + 1) // 2), 1 << (lg // 2), spp
    return 8, 8, 1


def scene(name):
    """(c, r, s, o, sh) float32 and the layers' index ranges, {"faint": (a, b), ...}"""
    if name in _CACHE:
        return _CACHE[name]
    p = SCENES[name]
    rng = np.random.default_rng(p["seed"])
    w, h = p["frame"]
    nf, nb, ns, nc, npin = p["faint"], p["opaque"], p["small"], p["clamped"], p.get("pins", 0)
    n = nf + nb + ns + nc + npin
    layer, at = {}, 0
    for key, k in (("faint", nf), ("opaque", nb), ("small", ns), ("clamped", nc), ("pins", npin)):
        layer[key] = (at, at + k)
        at += k
    half = math.tan(math.radians(FOVY / 2))  # the frame's half height at view depth 1
    px = 2.0 * half / h  # a pixel's width at view depth 1
    # view depths: faint, small and clamped share 4..12, the clamped ones in its middle third; the opaque layer 12.5..14
    z = np.zeros(n)
    front = n - nb
    mine = rng.choice(np.arange(front // 3, 2 * front // 3), nc, replace=False)  # the clamped ones' slots
    order = np.r_[rng.permutation(np.setdiff1d(np.arange(front), mine)), mine]
    idx = np.r_[np.arange(*layer["faint"]), np.arange(*layer["small"]), np.arange(*layer["pins"]),
                np.arange(*layer["clamped"])]
    z[idx] = 4.0 + 8.0 * (order + rng.uniform(0.25, 0.75, front)) / front
    z[slice(*layer["opaque"])] = 12.5 + 1.5 * (rng.permutation(nb) + rng.uniform(0.25, 0.75, nb)) / nb
    c = np.zeros((n, 3))
    s = np.zeros((n, 3))
    o = np.zeros(n)
    wide = np.r_[np.arange(*layer["faint"]), np.arange(*layer["opaque"])]
    c[wide, :2] = rng.uniform(-0.05, 0.05, (len(wide), 2)) * z[wide, None]
    s[wide] = rng.uniform(1.2, 1.5, (len(wide), 3)) * z[wide, None]
    o[slice(*layer["faint"])] = rng.uniform(*p["faint_o"], nf)
    o[slice(*layer["opaque"])] = rng.uniform(0.5, 0.7, nb)
    sm = np.arange(*layer["small"])
    c[sm, 0] = rng.uniform(-1.0, 1.0, ns) * half * w / h * z[sm]
    c[sm, 1] = rng.uniform(-1.0, 1.0, ns) * half * z[sm]
    s[sm] = (rng.uniform(*p["small_px"], ns) * px * z[sm])[:, None] * rng.uniform(0.8, 1.25, (ns, 3))
    o[sm] = rng.uniform(*p["small_o"], ns)
    # the clamped ones: on the ray of the first sample of a pixel, so that g ~ 0 there and o e = 1 > 0.99
    cl = np.arange(*layer["clamped"])
    u = F.Ubo(O.make_ubo(MV, FOVY, w, h, 1.0, 1, 16))
    jx, jy = F.jitter(u.seed, 1)[0]
    pix = rng.choice(w * h, nc, replace=False)
    _, d = F.rays(u, pix % w + jx, pix // w + jy)
    c[cl] = d * (z[cl] / -d[:, 2])[:, None]
    s[cl] = (1.0 * px * z[cl])[:, None] * np.ones(3)
    o[cl] = 1.0
    # the pins: on the ray of the second sample of a pixel, and so faint that alpha passes 1/255 only within half a pixel
    # of it (sigma^2 = 0.04 + 0.3 px^2, o e > 1/255 where g < 0.34): a pin's few dozen hits lie in one or two pixels, and
    # the second sample's, at e = 1, is the largest of them
    if npin:
        pn = np.arange(*layer["pins"])
        jx, jy = F.jitter(u.seed, 2)[1]
        pix = rng.choice(w * h, npin, replace=False)
        _, d = F.rays(u, pix % w + jx, pix // w + jy)
        c[pn] = d * (z[pn] / -d[:, 2])[:, None]
        s[pn] = (0.2 * px * z[pn])[:, None] * np.ones(3)
        o[pn] = 0.0055
    c[:, 2] = -z
    r = rng.standard_normal((n, 4))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    sh = rng.uniform(-0.01, 0.01, (n, 16, 3))
    pre0 = np.where(rng.random((n, 3)) < 0.69, rng.uniform(0.3, 1.2, (n, 3)), rng.uniform(-0.8, -0.3, (n, 3)))
    sh[:, 0, :] = (pre0 - 0.5) / F.SH_C0
    model = tuple(np.ascontiguousarray(a, np.float32) for a in (c, r, s, o, sh))
    assert len(np.unique(-model[0][:, 2])) == n  # distinct depths in float32
    _CACHE[name] = model + (layer,)
    return _CACHE[name]


def model(case, with_sh=True):
    c, r, s, o, sh, _ = scene(case[0])
    return c, r, s, o, (sh if with_sh else None)


def sensitive(case, with_sh=True):
    """the case's F.gradients without an upstream gradient: the float32-sensitive pixels and the event counts"""
    key = ("near", case, with_sh)
    if key not in _CACHE:
        _CACHE[key] = F.gradients(camera(case), *model(case, with_sh))
    return _CACHE[key]


def upstream(case, channels, seed, with_sh=True):
    """G (h, w, channels) float32: noise in -3..3, zero on the float32-sensitive pixels (as test_grad_f64.upstream)"""
    _, w, h, _ = case
    G = np.random.default_rng(seed).uniform(-3.0, 3.0, (w * h, channels)).astype(np.float32).reshape(h, w, channels)
    G[sensitive(case, with_sh).near] = 0.0
    return G


def upstream_depth(case, seed, with_sh=True):
    """Gdepth (h, w) float32: normal noise, zero on the sensitive pixels (as test_depth_grad_f64.upstream_depth)"""
    _, w, h, _ = case
    G = np.random.default_rng(seed).standard_normal((h, w)).astype(np.float32)
    G[sensitive(case, with_sh).near] = 0.0
    return G


def reference(case, with_sh=True):
    """G, F.gradients of it and F.render's frame, once per case (as test_grad_f64_gpu.reference)"""
    key = ("ref", case, with_sh)
    if key not in _CACHE:
        G = upstream(case, 4, 501 + case[3], with_sh)
        m = model(case, with_sh)
        _CACHE[key] = (G, F.gradients(camera(case), *m, G_rgba=G), F.render(camera(case), *m)[0])
    return _CACHE[key]


def feature_reference(case, channels):
    """Gf (h, w, channels), zero on the pixels sensitive without SH rows, and F.gradients of it"""
    key = ("feat", case, channels)
    if key not in _CACHE:
        G = upstream(case, channels, 601 + case[3], with_sh=False)
        _CACHE[key] = (G, F.gradients(camera(case), *model(case, False), G_feat=G))
    return _CACHE[key]


def splat_reference(case, with_sh=True):
    """reference's G and the float64 splat rows of it (cor_f64_geom.splat_gradients)"""
    key = ("splat", case, with_sh)
    if key not in _CACHE:
        G, ref, _ = reference(case, with_sh)
        sg = Q.splat_gradients(camera(case), *model(case, with_sh), G_rgba=G)
        assert sg.digest == ref.digest and np.array_equal(sg.near, ref.near)
        _CACHE[key] = (G, sg)
    return _CACHE[key]


def depth_reference(case, with_sh=True):
    """reference's G, Gdepth and the float64 splat-depth rows of both (cor_f64_depth.depth_gradients)"""
    key = ("depth", case, with_sh)
    if key not in _CACHE:
        G, ref, _ = reference(case, with_sh)
        Gd = upstream_depth(case, 701 + case[3], with_sh)
        dg = D.depth_gradients(camera(case), *model(case, with_sh), G_rgba=G, G_depth=Gd)
        assert dg.digest == ref.digest and np.array_equal(dg.near, ref.near)
        _CACHE[key] = (G, Gd, dg)
    return _CACHE[key]


def hit_sets(case):
    """(h * w, n) bool: the Gaussian has a hit the blend may take (inside its box, alpha > 1/255) on some sample ray of
    the pixel, by the reference's own selection (F._hits), and the hits per sample ray (h * w, spp). Whatever a renderer
    culls by, such a Gaussian is a candidate of the pixel's tile: the counts of these are a lower bound on the tile's and
    the group's, and the scene's size is the upper bound."""
    key = ("hits", case)
    if key not in _CACHE:
        c, r, s, o, sh, _ = scene(case[0])
        u = F.Ubo(camera(case))
        sp = F.Splats(u, c, r, s, o, None)
        ys, xs = np.mgrid[0:u.H, 0:u.W]
        xs, ys = xs.reshape(-1).astype(np.float64), ys.reshape(-1).astype(np.float64)
        has = np.zeros((u.H * u.W, sp.n), bool)
        per_ray = np.zeros((u.H * u.W, u.S), np.int64)
        everyone = np.arange(sp.n)
        for k, (jx, jy) in enumerate(F.jitter(u.seed, u.S)):
            o3, d = F.rays(u, xs + jx, ys + jy)
            h = F._hits(sp, everyone, xs + jx, ys + jy, o3, d, np.zeros(len(xs), bool), 1e-3, 1e-5, 1e-6)
            has[h.ri, h.gi] = True
            per_ray[:, k] = np.bincount(h.ri, minlength=len(xs))
        _CACHE[key] = (has, per_ray)
    return _CACHE[key]


def block_counts(case, bw, bh):
    """the number of Gaussians with a hit in each bw x bh block of pixels (ragged blocks at the frame's edges included)"""
    _, w, h, _ = case
    has = hit_sets(case)[0].reshape(h, w, -1)
    return np.array([[has[y:y + bh, x:x + bw].any((0, 1)).sum() for x in range(0, w, bw)] for y in range(0, h, bh)])


# ------------------------------------------------------------------------------------------------ planted faults
def _take(h, keep):
    """the hit lists h with the entries of the index array `keep`, in that order"""
    for k in ("ri", "gi", "alpha", "oe", "e", "col", "pre", "Y"):
        v = getattr(h, k)
        if v is not None:
            setattr(h, k, v[keep])
    return h


def _positions(ri):
    """every entry's position in its ray's list (the lists are contiguous, rays ascending)"""
    first = np.flatnonzero(np.r_[True, ri[1:] != ri[:-1]]) if len(ri) else np.zeros(0, np.int64)
    return np.arange(len(ri)) - np.repeat(first, np.diff(np.r_[first, len(ri)]))


@contextlib.contextmanager
def planted(fault):
    """F.gradients with one fault of a renderer that works in rounds of K_CAP entries and in passes, planted in a copy of
    the reference's hit lists (a position is an entry's index in its ray's list, in depth order):
      "drop256", "drop896"  the entries from position 256 / 896 on are dropped: the rounds after the first, or the group
                            list's second segment, never run;
      "skip257"             the entry at position 256 is dropped: the round after a cut resumes one entry late;
      "twice"               the entry at position 255 is blended twice: a round boundary hands its last entry on;
      "pass_twice"          the second sample's terms are added twice: with one sample per pass, a pass counted twice;
      "sweep_short"         the terms of a ray's last round are missing from the opacity gradient while everything those
                            of the earlier rounds are formed from (T, the colour behind a hit, the final T) is whole: the
                            second sweep of a resweep kind stops one round early, after a complete first sweep."""
    real_hits, real_walk, real_scatter, real_jitter = F._hits, F._walk, F._scatter, F.jitter
    state = {}

    def hits(*a, **k):
        h = real_hits(*a, **k)
        pos = _positions(h.ri)
        if fault == "drop256":
            _take(h, np.flatnonzero(pos < K_CAP))
        elif fault == "drop896":
            _take(h, np.flatnonzero(pos < K_GCAP))
        elif fault == "skip257":
            _take(h, np.flatnonzero(pos != K_CAP))
        elif fault == "twice":
            _take(h, np.sort(np.r_[np.arange(len(pos)), np.flatnonzero(pos == K_CAP - 1)], kind="stable"))
        return h

    def settled():  # every sample so far had its two opacity scatters (the gradient's and M's) rewritten, and no other
        assert state.get("rewritten", 2) == 2, state["rewritten"]
        state["rewritten"] = 0

    def walk(h, m, ray_near, trans_rel):
        settled()
        out = real_walk(h, m, ray_near, trans_rel)
        b = h.blended
        pos = _positions(h.ri[b])
        count = np.bincount(h.ri[b], minlength=m)[h.ri[b]]
        late = pos >= (count - 1) // K_CAP * K_CAP  # the ray's last round
        state["late_open"] = late[h.oe[b] < 0.99]
        return out

    def scatter(out, idx, val):
        late = state.get("late_open")
        if out.ndim == 1 and late is not None and len(late) == len(idx):  # the opacity gradient's terms, and M's
            val = np.where(late, 0.0, val)
            state["rewritten"] += 1
        real_scatter(out, idx, val)

    def jitter(seed, samples):
        j = real_jitter(seed, samples)
        return j + [j[1]]

    try:
        if fault == "sweep_short":
            F._walk, F._scatter = walk, scatter
        elif fault == "pass_twice":
            F.jitter = jitter
        else:
            assert fault in ("drop256", "drop896", "skip257", "twice"), fault
            F._hits = hits
        yield
        if fault == "sweep_short":
            settled()
    finally:
        F._hits, F._walk, F._scatter, F.jitter = real_hits, real_walk, real_scatter, real_jitter
