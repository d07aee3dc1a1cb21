"""SH colour frames shade a stage in two parts (weigh_hit, blend_stage in gsrt_render.hip): an ordered pass over alpha and
T that keeps each blend's weight, then per lane the SH colours of the candidates that lane blends, the lane's k-th blend
of the stage in pass k. Every frame here is byte-equal RGBA against the CPU oracle, and every scene asserts from the
oracle's per-ray counts (candidates, blends, stops) that blends do happen and, where the scene is about them, stops.

Scenes are small stacks of Gaussians in front of a camera at the origin looking down -z. A Gaussian's box is a cube of
three times its largest scale, so with scale 3 every ray meets every box and the tile's list is the stack.

Depth frames: the oracle has no depth output of its own, so its colour path carries it, as in test_depth_gpu.py: with
every centre at view depth exactly 4, depth = 4 x (the oracle's red channel of the same geometry without SH rows), bit
for bit; for the stacks at other depths, SH rows that encode z make the oracle's red channel the depth, within the
encoding's cost and one rounding per hit in each chain (a tolerance from the reference side only).
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
Y0 = np.float32(0.28209479177387814)  # the constant DC basis (kShY0)


def stack(k, opacity, scale=3.0, spread=0.0, seed=1, z0=-5.0, dz=0.01):
    """k Gaussians on the view axis at depths -z0, -z0 + dz, ... (sorted order = index order), isotropic `scale`,
    centres moved sideways by up to `spread` (uniform, seeded)."""
    rng = np.random.default_rng(seed)
    c = np.zeros((k, 3), np.float32)
    c[:, 2] = np.float32(z0) - np.float32(dz) * np.arange(k, dtype=np.float32)
    if spread:
        c[:, :2] = rng.uniform(-spread, spread, (k, 2)).astype(np.float32)
    r = np.tile(np.asarray(IDENT, np.float32), (k, 1))
    return c, r, np.full((k, 3), scale, np.float32), np.full(k, opacity, np.float32)


def sh_rows(k, seed=3):
    """SH-3 coefficients of the synthetic cloud (signed, so the clamp at 0 is met) for k Gaussians"""
    return gsrt.synth_cloud(gsrt.SYNTH_COR, max(k, 1), seed, True)[4][:k]


def depth_rows(z):
    """SH rows whose colour is (an encoding of) z in every channel, whatever the ray direction"""
    sh = np.zeros((len(z), 16, 3), np.float32)
    sh[:, 0, :] = ((np.asarray(z, np.float32) - np.float32(0.5)) / Y0)[:, None]
    return sh


def encoding_cost(z):
    s0 = depth_rows(z)[:, 0, 0]
    enc = (s0 * Y0).astype(np.float32) + np.float32(0.5)
    return float(np.abs(enc.astype(np.float64) - np.asarray(z, np.float64)).max())


def ubo_of(w, h, spp):
    return gsrt.camera_from_modelview(MV, FOV, w, h, 1.0, spp, 16)


_ORACLE = {}


def oracle_frame(key, model, sh, w, h, spp, lut=False):
    """(oracle rgba, per-pixel counts [candidates, blends, -, stops]); computed once per key and left unchanged"""
    if key not in _ORACLE:
        p, a = O.gauss_from_model(*model)
        ref = O.render(p, a, O.make_ubo(MV, FOV, w, h, 1.0, spp, 16), O.MODE_COR | (O.FLAG_LUT if lut else 0), sh=sh,
                       bvh=O.Bvh(a), want_stats=True, threads=4)
        rgba, st = ref["rgba"], ref["stats"].astype(np.int64)
        rgba.setflags(write=False)
        st.setflags(write=False)
        _ORACLE[key] = (rgba, st)
    return _ORACLE[key]


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


LIST_LENGTHS = [1, 3, 4, 5, 8, 9, 16, 17, 21]


@pytest.mark.parametrize("k", LIST_LENGTHS)
def test_list_lengths(ctx, k):
    """Lists of k entries in every tile of a 64x64 frame at 4 spp: every fill 1..4 of the last stage, lists shorter than
    the steady-state loop's entry (17) and one trip of it with a tail."""
    model, sh = stack(k, 0.05), sh_rows(k)
    want, st = oracle_frame(("lists", k), model, sh, 64, 64, 4)
    assert (st[..., 0] == k * 4).all() and (st[..., 3] == 0).all()  # every ray meets all k boxes and never stops
    assert st[..., 1].min() > 0                                      # and blends
    rgba, _ = gpu_frame(ctx, model, sh, 64, 64, 4)
    assert rgba.tobytes() == want.tobytes()


def half_tile_model():
    """Four stacked Gaussians, narrow in x and long in y, over two pixel columns right of the frame's centre column: in
    the 4x4-pixel tiles (one wave at 4 spp) that start at that column the left pixels blend all four, the right none."""
    k = 4
    px = 2.0 * 5.0 * np.tan(np.radians(FOV / 2)) / 16  # a pixel's width at depth 5 in a 16-pixel frame
    c, r, s, o = stack(k, 0.3)
    c[:, 0] = px
    s[:, 0], s[:, 1], s[:, 2] = px / 3.0, 3.0, 1e-3
    return c, r, s, o


def test_four_blends_on_some_lanes_none_on_others(ctx):
    model, sh = half_tile_model(), sh_rows(4, seed=5)
    w = h = 16
    pl = gsrt.tile_plan(ubo_of(w, h, 4))
    assert (pl["tile_w"], pl["tile_h"], pl["spp_lanes"]) == (4, 4, 4)
    want, st = oracle_frame("half", model, sh, w, h, 4)
    nblend = st[..., 1]
    mixed = 0
    for ty in range(0, h, 4):
        for tx in range(0, w, 4):
            t = nblend[ty:ty + 4, tx:tx + 4]
            # a pixel with 4 x 4 blends: each of its four lanes blends all four candidates of the stage
            mixed += int((t == K_GROUP * 4).any() and (t == 0).any())
    assert mixed >= 2
    rgba, _ = gpu_frame(ctx, model, sh, w, h, 4)
    assert rgba.tobytes() == want.tobytes()


STOPS = dict(k=22, opacity=0.99, scale=1.6, spread=1.3, seed=7)


@pytest.mark.parametrize("spp", [1, 4, 3])
def test_stops_inside_a_stage(ctx, spp):
    """Opacity 0.99, centres moved sideways: the rays of one wave stop at different candidates, at every position of a
    stage, while other lanes go on blending the stage's later candidates; a stopped lane blends nothing more."""
    k = STOPS["k"]
    model, sh = stack(**STOPS), sh_rows(k)
    want, st = oracle_frame(("stops", spp), model, sh, 16, 16, spp)
    ncand, nblend, nstop = st[..., 0], st[..., 1], st[..., 3]
    assert nstop.max() > 0 and nblend.max() > spp and (nblend > 0).mean() > 0.5
    if spp == 1:  # one ray per pixel: a ray that stops does so at list position ncand - 1
        stopped = nstop == 1
        assert (ncand[~stopped] == k).all() and stopped.sum() > 64
        pos = ncand - 1
        assert set((pos[stopped] % K_GROUP).tolist()) == {0, 1, 2, 3}
        found = False  # in one 8x8 tile (a wave): two rays stop in the same stage, the later after blending again
        for ty in range(0, 16, 8):
            for tx in range(0, 16, 8):
                m = stopped[ty:ty + 8, tx:tx + 8]
                pp, nb = pos[ty:ty + 8, tx:tx + 8][m], nblend[ty:ty + 8, tx:tx + 8][m]
                for stage in np.unique(pp // K_GROUP):
                    sel = pp // K_GROUP == stage
                    found |= np.unique(pp[sel]).size >= 2 and nb[sel].max() > nb[sel].min()
        assert found
    rgba, _ = gpu_frame(ctx, model, sh, 16, 16, spp)
    assert rgba.tobytes() == want.tobytes()


@pytest.mark.parametrize("spp,k", [(64, 9), (128, 6)])
def test_many_samples(ctx, spp, k):
    """64 spp: one pixel per wave; 128 spp at 16x16: two passes of a pixel per lane"""
    pl = gsrt.tile_plan(ubo_of(16, 16, spp))
    assert pl["spp_lanes"] == (64 if spp == 64 else 1)
    model, sh = stack(k, 0.4, scale=1.2, spread=0.8, seed=11), sh_rows(k)
    want, st = oracle_frame(("many", spp), model, sh, 16, 16, spp)
    assert st[..., 1].max() > spp and (st[..., 1] > 0).mean() > 0.5
    rgba, _ = gpu_frame(ctx, model, sh, 16, 16, spp)
    assert rgba.tobytes() == want.tobytes()


def test_continuation_round(ctx):
    """More than kCap contributing candidates in every tile of a 16x16 frame: a second round through the same loops"""
    k = 300
    model, sh = stack(k, 0.02, scale=6.0), sh_rows(k)
    want, st = oracle_frame("rounds", model, sh, 16, 16, 4)
    assert (st[..., 0] == k * 4).all() and (st[..., 3] == 0).all()
    assert st[..., 1].min() > K_CAP * 4
    rgba, _ = gpu_frame(ctx, model, sh, 16, 16, 4)
    assert rgba.tobytes() == want.tobytes()


def both_layouts_model(k=9):
    """The first Gaussian's box holds the camera (the general record layout); the others are small boxes in front of it
    in the octant x > 0, y > 0, z < 0 (the ordered layout)."""
    c, r, s, o = stack(k, 0.3)
    c[1:, :2] = 1.2
    s[1:] = 0.3
    return c, r, s, o


@pytest.mark.parametrize("spp", [4, 1])
def test_both_record_layouts(ctx, spp):
    k = 9
    model, sh = both_layouts_model(k), sh_rows(k)
    _, a = O.gauss_from_model(*model)
    inside = np.all((a[:, :3] < 0) & (a[:, 3:] > 0), axis=1)             # the camera origin inside the box
    one_sided = np.all((a[:, :3] > 0) | (a[:, 3:] < 0), axis=1)          # the box in one octant of the origin
    assert inside[0] and not one_sided[0] and one_sided[1:].all()
    want, st = oracle_frame(("layouts", spp), model, sh, 16, 16, spp)
    assert st[..., 0].max() == k * spp and st[..., 0].min() == spp  # rays through the small boxes meet both kinds
    assert st[..., 1].max() > 2 * spp and st[..., 1].min() > 0       # and blend both
    rgba, _ = gpu_frame(ctx, model, sh, 16, 16, spp)
    assert rgba.tobytes() == want.tobytes()


@pytest.mark.parametrize("scene", ["lists", "stops"])
def test_sh_lut_frame(ctx, scene):
    """The SH + LUT kernel (GSRT_FLAG_LUT) through the same two parts"""
    model = stack(17, 0.05) if scene == "lists" else stack(**STOPS)
    k = len(model[3])
    sh = sh_rows(k)
    want, st = oracle_frame(("lut", scene), model, sh, 16, 16, 4, lut=True)
    assert st[..., 1].min() > 0 and (st[..., 3].max() > 0) == (scene == "stops")
    rgba, _ = gpu_frame(ctx, model, sh, 16, 16, 4, lut=True)
    assert rgba.tobytes() == want.tobytes()


DEPTH_SCENES = {
    "lists5": lambda: stack(5, 0.05),
    "lists21": lambda: stack(21, 0.05),
    "half": half_tile_model,
    "stops": lambda: stack(**STOPS),
    "layouts": both_layouts_model,
    "rounds": lambda: stack(300, 0.02, scale=6.0),
}


@pytest.mark.parametrize("lut", [False, True])
@pytest.mark.parametrize("scene", list(DEPTH_SCENES))
def test_depth_frames(ctx, scene, lut):
    """GSRT_FLAG_DEPTH of the same scenes with SH rows (the depth SH kernels). RGBA byte-equal to the oracle; depth against
    the oracle's red channel of rows that encode z: tol = encoding cost + 2 n_max 2^-24 z_max (one fma rounding per hit in
    each of the two chains), n_max a bound on the oracle's largest per-ray blend count. With the scene's own SH colours
    the same hits are blended with the same weights: the same depth bits."""
    model = DEPTH_SCENES[scene]()
    k = len(model[3])
    z = -model[0][:, 2]
    rows = depth_rows(z)
    w = h = 16
    want, st = oracle_frame(("depth", scene, lut), model, rows, w, h, 4, lut=lut)
    assert st[..., 1].max() > 0
    n_max = min(k, int(st[..., 1].max()))  # a ray blends at most its pixel's count (summed over the samples), and k
    tol = encoding_cost(z) + 2.0 * n_max * 2.0 ** -24 * float(z.max())
    rgba, depth = gpu_frame(ctx, model, rows, w, h, 4, lut=lut, depth=True)
    assert rgba.tobytes() == want.tobytes()
    linf = float(np.abs(depth.astype(np.float64) - want[..., 0].astype(np.float64)).max())
    print(f"{scene} lut {lut}: depth vs oracle L-inf {linf:.3g}, tol {tol:.3g} (n_max {n_max})")
    assert linf <= tol
    assert not u32(depth)[want[..., 3] == 0].any()  # no blend: exactly +0
    sh = sh_rows(k)
    want2, _ = oracle_frame(("depth-own", scene, lut), model, sh, w, h, 4, lut=lut)
    rgba2, depth2 = gpu_frame(ctx, model, sh, w, h, 4, lut=lut, depth=True)
    assert rgba2.tobytes() == want2.tobytes()
    assert np.array_equal(u32(depth2), u32(depth))


@pytest.mark.parametrize("spp", [4, 3])
def test_depth_plane_is_exact(ctx, spp):
    """Every centre at view depth exactly 4 (z0 = -4, dz = 0), stops inside stages: depth = 4 x sum w bit for bit, sum w
    being the oracle's red channel of the same geometry without SH rows (colour 1); a power-of-two scale commutes with
    every rounding of the chain."""
    k = STOPS["k"]
    model, sh = stack(**STOPS, z0=-4.0, dz=0.0), sh_rows(k)
    assert (model[0][:, 2] == np.float32(-4.0)).all()
    sum_w, st = oracle_frame(("plane", spp), model, None, 16, 16, spp)
    assert st[..., 3].max() > 0 and st[..., 1].max() > spp
    want, _ = oracle_frame(("plane-sh", spp), model, sh, 16, 16, spp)
    rgba, depth = gpu_frame(ctx, model, sh, 16, 16, spp, depth=True)
    assert rgba.tobytes() == want.tobytes()
    assert np.array_equal(u32(depth), u32(np.float32(4.0) * sum_w[..., 0]))
