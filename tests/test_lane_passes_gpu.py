"""SH colour frames run phase 2 of a stage per lane (lane_pass, shade_lanes in gsrt_render.hip): pass J handles every
lane's J-th g-passing candidate of the stage end to end: record read at the lane's own address, slab test, exp, alpha, T,
stop and, where the lane blends, the SH row and the colour. The change reorders no float operation, so every frame here
is byte-equal against the CPU oracle (oracle.render, MODE_COR): RGBA always, and the depth image of depth frames.

What a scene is about is shown by the oracle alone, at 1 spp, where a pixel's counts [candidates, blends, -, stops] are
one ray's. `alone(i)` is the oracle's frame of Gaussian i by itself: a ray blends it there exactly when the pair (ray,
candidate) passes the slab test, g and alpha > 1/255 (T = 1, and alpha <= 0.99 never stops a fresh ray), whatever the
other candidates do. A list is sorted by view depth, which falls with the index in every scene, so list position = index
and a stage is four consecutive indices. Ranks inside a stage are counted over these full passes; g-passing is the
wider set by the margin between gcut and alpha > 1/255 (g within 0.01) and by lanes that pass g outside the box.

Depth frames: the oracle has no depth output, so its colour path carries it as in test_depth_gpu.py. The `flat` variant
of a scene puts every centre at view depth exactly 4 (ties keep index order); then depth = 4 x sum w bit for bit, sum w
being the oracle's red channel of the same geometry without SH rows (colour 1): a power-of-two scale commutes with every
rounding of the fma chain.
"""
import numpy as np
import pytest

import gsrt
import oracle as O

pytestmark = pytest.mark.gpu

K_GROUP = 4   # candidates per LDS stage (kGroup)
K_CAP = 256   # list entries per round (kCap)
FOV = 60.0
IDENT = (1.0, 0.0, 0.0, 0.0)
MV = gsrt.lookat((0, 0, 0), (0, 0, -1))


def model_of(centres, scales, opacities, flat=False):
    c = np.asarray(centres, np.float32).reshape(-1, 3).copy()
    k = len(c)
    if flat:
        c[:, 2] = np.float32(-4.0)
    s = np.asarray(scales, np.float32)
    s = np.tile(s, (k, 1)) if s.ndim == 1 and s.size == 3 else np.broadcast_to(s.reshape(k, -1), (k, 3)).copy()
    o = np.broadcast_to(np.asarray(opacities, np.float32), (k,)).copy()
    return c, np.tile(np.asarray(IDENT, np.float32), (k, 1)), s, o


def stack(k, opacity, scale=3.0, spread=0.0, seed=1, flat=False):
    """k Gaussians on the view axis at depths 5, 5.01, ... (list order = index order), centres moved sideways by up to
    `spread` (uniform, seeded). Scale 3: every ray meets every box."""
    rng = np.random.default_rng(seed)
    c = np.zeros((k, 3), np.float32)
    c[:, 2] = np.float32(-5.0) - np.float32(0.01) * np.arange(k, dtype=np.float32)
    if spread:
        c[:, :2] = rng.uniform(-spread, spread, (k, 2)).astype(np.float32)
    return model_of(c, [scale] * 3, opacity, flat)


def mixed_model(flat=False):
    """Small boxes in one octant of the camera (the ordered record layout) between boxes that straddle the camera's
    x = 0 and y = 0 planes (the general layout), all in the first stage; two more of each behind."""
    c = [(0.9, 0.9, -5.00), (0.0, 0.0, -5.01), (-0.9, 0.9, -5.02), (0.0, 1.5, -5.03),
         (0.9, -0.9, -5.04), (0.0, 0.0, -5.05), (-0.9, -0.9, -5.06), (1.5, 0.0, -5.07)]
    s = [(0.2, 0.2, 0.2), (3, 3, 1), (0.2, 0.2, 0.2), (1.0, 0.3, 0.3),
         (0.2, 0.2, 0.2), (3, 3, 1), (0.2, 0.2, 0.2), (0.3, 1.0, 0.3)]
    return model_of(c, s, 0.3, flat)


def half_tile_model(flat=False):
    """Four stacked Gaussians, narrow in x and long in y, over two pixel columns right of the frame's centre column: in
    the tiles that start at that column some pixels pass all four candidates of the stage, others none."""
    px = 2.0 * 5.0 * np.tan(np.radians(FOV / 2)) / 16  # a pixel's width at depth 5 in a 16-pixel frame
    c = [(px, 0.0, -5.0 - 0.01 * i) for i in range(4)]
    return model_of(c, (px / 3.0, 3.0, 1e-3), 0.3, flat)


def stops_model(flat=False):
    """Opaque Gaussians whose centres are moved sideways: a ray's alpha differs from candidate to candidate and from pixel
    to pixel, so the rays of one wave stop at different candidates while others go on."""
    return stack(12, 0.99, scale=1.6, spread=1.3, seed=7, flat=flat)


def ring_model(flat=False):
    """Candidate 0 is small and faint between rays that blend it and rays that do not; three wide candidates behind it.
    With the LUT the g test is g <= 5.6 for every candidate, so at opacity 0.05 the rays with 2.55 < g <= 5.6 pass g and
    the slab test and fail alpha > 1/255. Candidate 2 is small and opaque: g <= ln(255 x 0.99) + 0.01 reaches 3.33 sigma,
    its box 3 sigma, so rays along the box's sides pass g and miss the box."""
    c = [(0.3, 0.2, -5.00), (0.0, 0.0, -5.01), (-0.5, -0.4, -5.02), (0.0, 0.0, -5.03)]
    s = [(0.5, 0.5, 0.5), (3, 3, 1), (0.45, 0.45, 0.45), (3, 3, 1)]
    return model_of(c, s, [0.05, 0.3, 0.99, 0.3], flat)


SCENES = {"mixed": mixed_model, "half": half_tile_model, "stops": stops_model, "ring": ring_model}
LIST_LENGTHS = [1, 3, 4, 5, 17, 300]


def scene_model(name, flat=False):
    if name.startswith("list"):
        k = int(name[4:])
        return stack(k, 0.02 if k > K_CAP else 0.05, scale=6.0 if k > K_CAP else 3.0, flat=flat)
    return SCENES[name](flat)


def sh_rows(k, seed=3):
    """SH-3 coefficients of the synthetic cloud (signed, so the clamp at 0 is met) for k Gaussians"""
    return gsrt.synth_cloud(gsrt.SYNTH_COR, max(k, 1), seed, True)[4][:k]


def ubo_of(w, h, spp):
    return gsrt.camera_from_modelview(MV, FOV, w, h, 1.0, spp, 16)


_ORACLE = {}


def oracle_frame(key, model, sh, w, h, spp, lut=False):
    """(oracle rgba, per-pixel counts [candidates, blends, -, stops]); computed once per key and left unchanged"""
    key = (key, w, h)
    if key not in _ORACLE:
        p, a = O.gauss_from_model(*model)
        ref = O.render(p, a, O.make_ubo(MV, FOV, w, h, 1.0, spp, 16), O.MODE_COR | (O.FLAG_LUT if lut else 0), sh=sh,
                       bvh=O.Bvh(a), want_stats=True, threads=4)
        rgba, st = ref["rgba"], ref["stats"].astype(np.int64)
        rgba.setflags(write=False)
        st.setflags(write=False)
        _ORACLE[key] = (rgba, st)
    return _ORACLE[key]


def alone(name, model, i, w, h, lut=False, opacity=None):
    """The oracle's 1-spp counts of Gaussian i by itself (optionally at another opacity): (slab hit, blends), bool H x W"""
    one = tuple(x[i:i + 1].copy() for x in model)
    if opacity is not None:
        one[3][:] = opacity
    _, st = oracle_frame(("alone", name, i, w, h, lut, opacity), one, None, w, h, 1, lut=lut)
    return st[..., 0] > 0, st[..., 1] > 0


def gpu_frame(ctx, model, sh, w, h, spp, lut=False, depth=False):
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        mode = gsrt.MODE_COR | (gsrt.FLAG_LUT if lut else 0)
        if depth:
            return sc.render_depth(ubo_of(w, h, spp), mode)
        return sc.render(ubo_of(w, h, spp), mode)[0], None
    finally:
        sc.close()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tiles(w, h, spp):
    """the pixel rectangles one wave shades"""
    pl = gsrt.tile_plan(ubo_of(w, h, spp))
    tw, th = pl["tile_w"], pl["tile_h"]
    assert tw * th * pl["spp_lanes"] == 64
    return [(slice(y, y + th), slice(x, x + tw)) for y in range(0, h, th) for x in range(0, w, tw)]


def size_of(name):
    return (32, 32) if name.startswith("ring") else (16, 16)


# ---- what each scene is about, from the oracle at 1 spp (one ray per pixel, one wave per 8x8 pixels)

def check_mixed(name, model, lut):
    w, h = size_of(name)
    _, a = O.gauss_from_model(*model)
    one_sided = np.all((a[:, :3] > 0) | (a[:, 3:] < 0), axis=1)  # the box in one octant of the origin: ordered layout
    assert one_sided[[0, 2, 4, 6]].all() and not one_sided[[1, 3, 5, 7]].any()
    passes = np.stack([alone(name, model, i, w, h, lut)[1] for i in range(len(a))])  # [candidate, y, x]
    found = 0
    for t in tiles(w, h, 1):
        for stage in range(0, len(a), K_GROUP):
            p = passes[stage:stage + K_GROUP][(slice(None),) + t].reshape(K_GROUP, -1)  # [candidate of the stage, lane]
            rank = np.cumsum(p, axis=0) - 1
            for j in range(K_GROUP):  # the layouts of the lanes' j-th candidates
                kinds = {bool(one_sided[stage + c]) for c in range(K_GROUP) if (p[c] & (rank[c] == j)).any()}
                found += len(kinds) == 2
    assert found >= 2  # a pass whose lanes hold records of both layouts


def check_half(name, model, lut):
    w, h = size_of(name)
    passes = np.stack([alone(name, model, i, w, h, lut)[1] for i in range(4)])
    found = 0
    for t in tiles(w, h, 1):
        p = passes[(slice(None),) + t]
        # all four on one lane, none on another (the boxes are cubes of the long y scale, so every ray meets them: the
        # lanes that pass none fail g, columns away from a footprint a third of a pixel wide in sigma)
        found += bool(p.all(axis=0).any() and (~p.any(axis=0)).any())
    assert found >= 1


def check_stops(name, model, lut):
    w, h = size_of(name)
    k = len(model[3])
    _, st = oracle_frame((name, False, 1, lut), model, sh_rows(k), w, h, 1, lut=lut)
    ncand, nstop = st[..., 0], st[..., 3]
    stopped = nstop == 1
    assert (ncand[~stopped] == k).all() and stopped.sum() > 32  # every ray meets every box: a stop is at ncand - 1
    passes = np.stack([alone(name, model, i, w, h, lut)[1] for i in range(k)])
    ranks = set()
    for y, x in zip(*np.nonzero(stopped)):
        pos = int(ncand[y, x]) - 1
        s0 = pos - pos % K_GROUP
        p = passes[s0:min(s0 + K_GROUP, k), y, x]
        if p[pos - s0] and p[pos - s0 + 1:].any():  # it stops here and would pass a later candidate of the stage
            ranks.add(int(p[:pos - s0].sum()))
    assert {0, 1, 2} <= ranks  # a stop in the lane's first, second and third pass of a stage


def check_ring(name, model, lut):
    w, h = size_of(name)
    k = len(model[3])
    _, st = oracle_frame((name, False, 1, lut), model, sh_rows(k), w, h, 1, lut=lut)
    assert (st[..., 3] == 0).all()
    hit2, _ = alone(name, model, 2, w, h, lut)
    edge = sum(bool(hit2[t].any() and (~hit2[t]).any()) for t in tiles(w, h, 1))
    assert edge >= 1  # candidate 2's box ends inside a wave: lanes beside it miss the box
    if lut:
        # blends at opacity 0.99 (g <= 5.53 and the box) and not at its own 0.05: passes g <= 5.6 and the slab test, fails
        # alpha > 1/255; the wide candidates 1 and 3 behind it still blend
        _, hi = alone(name, model, 0, w, h, True, opacity=0.99)
        _, lo = alone(name, model, 0, w, h, True)
        _, p1 = alone(name, model, 1, w, h, True)
        _, p3 = alone(name, model, 3, w, h, True)
        faint = hi & ~lo
        assert faint.sum() >= 8 and (p1 & p3)[faint].all() and (st[..., 1][faint] >= 2).all()
        assert sum(bool(faint[t].any() and lo[t].any()) for t in tiles(w, h, 1)) >= 1  # beside lanes that blend it


CHECKS = {"mixed": check_mixed, "half": check_half, "stops": check_stops, "ring": check_ring}


def check_lists(name, st, spp):
    k = int(name[4:])
    assert (st[..., 0] == k * spp).all() and (st[..., 3] == 0).all()  # every ray meets all k boxes and never stops
    assert st[..., 1].min() > (K_CAP * spp if k > K_CAP else 0)      # blends; k > kCap: into a continuation round


ALL = list(SCENES) + [f"list{k}" for k in LIST_LENGTHS]
# every scene at 1 and 4 spp in the plain kernel; the LUT and the two depth kernels: every scene at 4 spp, the scenes with
# a condition also at 1 spp; one case at 3 spp (several passes of a pixel per lane)
CASES = [(n, spp, False) for n in ALL for spp in (1, 4)] + [(n, 4, True) for n in ALL] + \
        [(n, 1, True) for n in SCENES] + [("stops", 3, False)]


@pytest.mark.parametrize("name,spp,lut", CASES)
def test_colour_frame(ctx, name, spp, lut):
    model = scene_model(name)
    k = len(model[3])
    w, h = size_of(name)
    if name in CHECKS:
        CHECKS[name](name, model, lut)
    sh = sh_rows(k)
    want, st = oracle_frame((name, False, spp, lut), model, sh, w, h, spp, lut=lut)
    if name.startswith("list"):
        check_lists(name, st, spp)
    assert st[..., 1].max() > 0
    rgba, _ = gpu_frame(ctx, model, sh, w, h, spp, lut=lut)
    assert rgba.tobytes() == want.tobytes()


DEPTH_CASES = [(n, 4, lut) for n in ALL for lut in (False, True)] + [(n, 1, lut) for n in SCENES for lut in (False, True)] + \
              [("stops", 3, False)]


@pytest.mark.parametrize("name,spp,lut", DEPTH_CASES)
def test_depth_frame(ctx, name, spp, lut):
    """The flat variant of every scene (all centres at view depth exactly 4): RGBA byte-equal to the oracle, depth
    byte-equal to 4 x the oracle's sum of weights."""
    model = scene_model(name, flat=True)
    assert (model[0][:, 2] == np.float32(-4.0)).all()
    k = len(model[3])
    w, h = size_of(name)
    if name in CHECKS:
        CHECKS[name](name + "-flat", model, lut)
    sh = sh_rows(k)
    want, st = oracle_frame((name + "-flat", False, spp, lut), model, sh, w, h, spp, lut=lut)
    sum_w, _ = oracle_frame((name + "-flat", True, spp, lut), model, None, w, h, spp, lut=lut)
    if name.startswith("list"):
        check_lists(name, st, spp)
    assert st[..., 1].max() > 0
    rgba, depth = gpu_frame(ctx, model, sh, w, h, spp, lut=lut, depth=True)
    assert rgba.tobytes() == want.tobytes()
    assert np.array_equal(u32(depth), u32(np.float32(4.0) * sum_w[..., 0]))
