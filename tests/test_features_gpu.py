"""Feature frames (GSRT_FLAG_FEATURES, include/gsrt.h): F_c = sum of f_c w over each ray's blended hits, f the scene's
per-Gaussian feature table, w = alpha T the colour blend's own weight, combined over a pixel's samples exactly as the
colour is; the frame's RGBA is that of the same geometry without SH rows.

References, none of which needed a change to the oracle:
  * constant channels: channel k = 2^(k-8) everywhere must equal 2^(k-8) x (the red channel of the no-SH plain frame,
    where colour is 1 and red = sum w), bit for bit: a power-of-two scale commutes with every rounding of the chain;
  * the depth image: a channel holding -c_z under the origin camera is the depth frame's z, so the bits are equal;
  * the oracle's colour path, three channels at a time: SH rows with s_k = 0 for k >= 1 and s_0 = (f - 0.5) / Y0 make
    channel ch's colour fl(fl(s_0 Y0) + 0.5) ~ f_ch (non-negative features only: the colour is clamped at 0);
  * tests/cor_f64.py, the independent float64 restatement, given the same rows in float64.

Every frame here is at most 64x48 pixels over at most 20k Gaussians.
"""
import ctypes
import os

import numpy as np
import pytest

import cor_f64 as F
import gsrt
import oracle as O

pytestmark = pytest.mark.gpu

FOV = 60.0
IDENT = (1.0, 0.0, 0.0, 0.0)
Y0 = np.float32(0.28209479177387814)  # the constant DC basis (kShY0, oracle sh_basis bs[0])
K_GROUP, K_CAP, K_GLIST = 4, 256, 896  # candidates per LDS stage, list entries per round, keys of a group list
MV = gsrt.lookat((0, 0, 0), (0, 0, -1))


def ubo_of(w, h, spp, mv=MV):
    return gsrt.camera_from_modelview(mv, FOV, w, h, 1.0, spp, 16)


def feature_rows(f3, dtype=np.float32):
    """SH rows whose colour is (an encoding of) the three columns of f3, whatever the ray direction"""
    f3 = np.asarray(f3, dtype)
    sh = np.zeros((len(f3), 16, 3), dtype)
    sh[:, 0, :] = (f3 - dtype(0.5)) / dtype(Y0)
    return sh


def encoding_cost(f3):
    """the largest |fl(fl(s0 Y0) + 0.5) - f| over the table, in float32: what the rows' encoding of f costs"""
    s0 = feature_rows(f3)[:, 0, :]
    enc = (s0 * Y0).astype(np.float32) + np.float32(0.5)
    return float(np.abs(enc.astype(np.float64) - np.asarray(f3, np.float64)).max())


def synth_sh(k, seed=3):
    return gsrt.synth_cloud(gsrt.SYNTH_COR, max(k, 1), seed, True)[4][:k]


def plane(k, opacity, scale, spread=0.0, seed=7):
    """k Gaussians whose centres all lie in the plane z = -4 (view depth exactly 4 from the origin camera), isotropic
    `scale`, moved sideways by up to `spread` (uniform, seeded)."""
    rng = np.random.default_rng(seed)
    c = np.zeros((k, 3), np.float32)
    c[:, 2] = -4.0
    if spread:
        c[:, :2] = rng.uniform(-spread, spread, (k, 2)).astype(np.float32)
    r = np.tile(np.asarray(IDENT, np.float32), (k, 1))
    return c, r, np.full((k, 3), scale, np.float32), np.full(k, opacity, np.float32)


PLANES = {
    "one": dict(k=1, opacity=0.8, scale=0.3),
    "stops": dict(k=22, opacity=0.99, scale=1.6, spread=1.3),
    "rounds": dict(k=300, opacity=0.02, scale=6.0),
    "past_group_list": dict(k=1500, opacity=0.006, scale=6.0),
}


def oracle_frame(model, sh, w, h, spp, lut=False, mv=MV):
    p, a = O.gauss_from_model(*model)
    ref = O.render(p, a, O.make_ubo(mv, FOV, w, h, 1.0, spp, 16), O.MODE_COR | (O.FLAG_LUT if lut else 0), sh=sh,
                   bvh=O.Bvh(a), want_stats=True, threads=4)
    return ref["rgba"], ref["stats"].astype(np.int64)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _cloud(name):
    if name == "sh3_1k":
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cor_sh3_1k.npz"))
        model, sh, shape = (z["center"], z["rot"], z["scale"], z["opacity"]), z["sh"], (48, 32, 4)
    elif name == "10k":
        c, r, s, o, _ = gsrt.synth_cloud(gsrt.SYNTH_COR, 10000, 42, False)
        model, sh, shape = (c, r, s, o), None, (64, 48, 1)
    else:
        c, r, s, o, _ = gsrt.synth_cloud(gsrt.SYNTH_COR, 20000, 7, False)
        model, sh, shape = (c, r, s, o), None, (64, 48, 3)
    return tuple(np.ascontiguousarray(a, np.float32) for a in model), sh, shape


def noise(n, channels, seed, lo=-3.0, hi=3.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, channels)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ 1: constant channels
@pytest.mark.parametrize("spp", [1, 4, 3])
@pytest.mark.parametrize("size", [16, 18])
@pytest.mark.parametrize("name", list(PLANES))
def test_constant_channels_are_exact(ctx, name, size, spp):
    """16 channels, channel k constant at 2^(k-8): channel k == 2^(k-8) x (sum w), bit for bit, with and without the LUT
    (the two FEAT instantiations of k_render_cor), for scenes with and without SH rows, through stops inside a stage,
    continuation rounds, the group list's end and, at 3 spp, the multi-pass path. The feature frame's rgba is the no-SH
    plain frame's and the oracle's no-SH frame, byte for byte, even when the scene has SH rows."""
    model = plane(**PLANES[name])
    k = len(model[3])
    ubo = ubo_of(size, size, spp)
    pl = gsrt.tile_plan(ubo)
    assert (pl["spp_lanes"] != spp) == (spp == 3)  # 3 spp run as passes, 1 and 4 in the wave
    scale = np.float32(2.0) ** np.arange(-8, 8, dtype=np.float32)
    table = np.tile(scale, (k, 1))
    plain = {}
    for with_sh in (False, True):
        sc = gsrt.Scene.from_model(ctx, *model, synth_sh(k) if with_sh else None)
        try:
            sc.build_bvh()
            sc.set_features(table)
            assert sc.features() == 16
            for lut in (False, True):
                mode = gsrt.MODE_COR | (gsrt.FLAG_LUT if lut else 0)
                label = f"{name} {size}x{size} spp {spp} sh {with_sh} lut {lut}"
                if not with_sh:
                    plain[lut], _ = sc.render(ubo, mode)
                    want, st = oracle_frame(model, None, size, size, spp, lut)
                    assert plain[lut].tobytes() == want.tobytes(), label
                    # the scene still does what it is here for
                    nblend, nstop = st[..., 1], st[..., 3]
                    if name == "one":
                        assert (want[..., 3] == 0).any() and (want[..., 3] > 0).any()
                    elif name == "stops":
                        assert nstop.max() > 0
                        if spp == 1:  # one ray per pixel: a stop at list position ncand - 1
                            pos = (st[..., 0] - 1)[nstop == 1]
                            assert set((pos % K_GROUP).tolist()) == {0, 1, 2, 3}
                    elif name == "rounds":
                        assert nblend.min() > K_CAP * spp
                    else:
                        assert nblend.min() > K_GLIST * spp
                rgba, feat = sc.render_features(ubo, mode)
                assert feat.shape == (size, size, 16)
                assert rgba.tobytes() == plain[lut].tobytes(), label  # colour 1, whatever the scene's SH rows
                assert np.array_equal(u32(rgba[..., 0]), u32(rgba[..., 1])), label
                assert np.array_equal(u32(rgba[..., 0]), u32(rgba[..., 2])), label
                sum_w = plain[lut][..., 0]
                assert np.array_equal(u32(feat), u32(sum_w[..., None] * scale)), label
                assert not u32(feat)[rgba[..., 3] == 0].any(), label  # no blend: exactly +0
        finally:
            sc.close()


# ------------------------------------------------------------------------------------------------ 2: depth as a feature
@pytest.mark.parametrize("channels", [1, 5, 16])
@pytest.mark.parametrize("name", ["sh3_1k", "10k", "20k"])
def test_feature_of_view_depth_is_the_depth_image(ctx, name, channels):
    """Under the origin camera a Gaussian's view depth is -c_z exactly: a channel holding it, among seeded noise, has
    the depth frame's bits (the same fma chain over the same hits with the same weights)."""
    model, sh, (w, h, spp) = _cloud(name)
    ubo = ubo_of(w, h, spp)
    at = channels // 2
    table = noise(len(model[3]), channels, 17)
    table[:, at] = -model[0][:, 2]
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        _, depth = sc.render_depth(ubo)
        sc.set_features(table)
        rgba, feat = sc.render_features(ubo)
    finally:
        sc.close()
    assert feat.shape == (h, w, channels)
    assert (rgba[..., 3] > 0).mean() > 0.5 and depth.max() > 1.0
    assert np.array_equal(u32(feat[..., at]), u32(depth))


# ------------------------------------------------------------------------------------------------ 3: independence
@pytest.fixture(scope="module")
def wide():
    """the 20k cloud (3 spp: passes) and a 16-channel table; the 16-channel frame is rendered once (by the first user)"""
    model, _, shape = _cloud("20k")
    return dict(model=model, shape=shape, table=noise(len(model[3]), 16, 23), frame=None)


def _wide_frame(ctx, wide):
    if wide["frame"] is None:
        sc = gsrt.Scene.from_model(ctx, *wide["model"])
        sc.build_bvh()
        sc.set_features(wide["table"])
        wide["frame"] = sc.render_features(ubo_of(*wide["shape"]))
        sc.close()
    return wide["frame"]


@pytest.mark.parametrize("channels", [1, 3, 7])
def test_channels_are_independent_and_the_store_writes_only_c(ctx, wide, channels):
    """The first C columns of a 16-channel table rendered as a C-channel table give the 16-channel frame's first C
    channels, bit for bit; and a device output of H*W*C + 64 floats keeps its 64 trailing sentinels."""
    import torch

    w, h, spp = wide["shape"]
    ubo = ubo_of(w, h, spp)
    rgba16, feat16 = _wide_frame(ctx, wide)
    sc = gsrt.Scene.from_model(ctx, *wide["model"])
    try:
        sc.build_bvh()
        sc.set_features(wide["table"][:, :channels])
        rgba, feat = sc.render_features(ubo)
        assert rgba.tobytes() == rgba16.tobytes()
        assert np.array_equal(u32(feat), u32(feat16[..., :channels]))
        sentinel = np.float32(-12345.5)
        d_feat = torch.full((h * w * channels + 64,), float(sentinel), dtype=torch.float32, device="cuda:0")
        gsrt._check(gsrt.lib.gsrt_render_features(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0, None,
                                                  ctypes.c_void_p(d_feat.data_ptr())), ctx)
        got = d_feat.cpu().numpy()
        assert got[:h * w * channels].tobytes() == feat.tobytes()
        assert (got[h * w * channels:] == sentinel).all()
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------ 4: sign, non-finite
def test_negated_table_negates_the_image(ctx):
    model, _, (w, h, spp) = _cloud("10k")
    table = noise(len(model[3]), 5, 29, 0.25, 3.0)  # no zero feature: no +0 product whose negation is -0 + 0
    ubo = ubo_of(w, h, 4)
    sc = gsrt.Scene.from_model(ctx, *model)
    try:
        sc.build_bvh()
        sc.set_features(table)
        rgba, pos = sc.render_features(ubo)
        sc.set_features(-table)
        rgba2, neg = sc.render_features(ubo)
    finally:
        sc.close()
    assert rgba.tobytes() == rgba2.tobytes()
    hit = rgba[..., 3] > 0
    assert hit.any() and (pos[hit] > 0).all()
    assert np.array_equal(u32(neg)[hit], u32(pos)[hit] ^ np.uint32(0x80000000))
    assert not u32(neg)[~hit].any() and not u32(pos)[~hit].any()


@pytest.mark.parametrize("spp", [1, 4, 3])
def test_infinite_feature_passes_through(ctx, spp):
    model = plane(**PLANES["one"])
    ubo = ubo_of(18, 18, spp)
    sc = gsrt.Scene.from_model(ctx, *model)
    try:
        sc.build_bvh()
        sc.set_features(np.array([[1.0, np.inf, -np.inf]], np.float32))
        rgba, feat = sc.render_features(ubo)
    finally:
        sc.close()
    hit = rgba[..., 3] > 0
    assert hit.any() and (~hit).any()
    assert np.array_equal(u32(feat[..., 0]), u32(rgba[..., 0]))
    assert (feat[..., 1][hit] == np.inf).all() and (feat[..., 2][hit] == -np.inf).all()
    assert not u32(feat)[~hit].any()


# ------------------------------------------------------------------------------------------------ 5: the oracle
@pytest.mark.parametrize("name", ["10k", "20k"])
def test_features_of_clouds_match_the_oracle(ctx, name):
    """Six non-negative channels in [0, 8] against the oracle's frames coloured by three of them at a time. Tolerance
    from the reference side only: tol = delta + 2 n_max 2^-24 f_max, delta the rows' encoding cost, n_max the oracle's
    largest per-pixel blend count (one fma rounding per hit in each of the two chains). Every pixel is asserted."""
    model, _, (w, h, spp) = _cloud(name)
    table = noise(len(model[3]), 6, 31, 0.0, 8.0)
    ubo = ubo_of(w, h, spp)
    sc = gsrt.Scene.from_model(ctx, *model)
    sc.build_bvh()
    sc.set_features(table)
    plain, _ = sc.render(ubo, gsrt.MODE_COR)
    rgba, feat = sc.render_features(ubo)
    sc.close()
    assert rgba.tobytes() == plain.tobytes()
    assert (rgba[..., 3] > 0).mean() > 0.5 and feat.max() > 1.0
    f_max = float(table.max())
    for g in range(2):
        cols = table[:, 3 * g:3 * g + 3]
        want, st = oracle_frame(model, feature_rows(cols), w, h, spp)
        assert np.array_equal(u32(want[..., 3]), u32(rgba[..., 3]))  # the same hits
        tol = encoding_cost(cols) + 2.0 * float(st[..., 1].max()) * 2.0 ** -24 * f_max
        linf = float(np.abs(feat[..., 3 * g:3 * g + 3].astype(np.float64) - want[..., :3].astype(np.float64)).max())
        print(f"{name} channels {3 * g}..{3 * g + 2}: features vs oracle L-inf {linf:.3g}, tol {tol:.3g} "
              f"(n_max {st[..., 1].max()}, f_max {f_max:.4g})")
        assert linf <= tol


# ------------------------------------------------------------------------------------------------ 6: float64
@pytest.mark.parametrize("cam", ["origin", "moved"])
def test_features_match_f64(ctx, cam):
    """Against the independent float64 restatement given the feature rows in float64: L-inf <= 1e-3 f_max on every
    pixel and channel (the project's 1e-3 criterion applied per channel); the float32-sensitive share is reported, not
    excluded."""
    (c, r, s, o), _, (w, h, spp) = _cloud("10k")
    mv = MV if cam == "origin" else gsrt.lookat((0.3, -0.2, 0.5), (0.1, 0.05, -1.0))
    ubo = ubo_of(w, h, spp, mv)
    table = noise(len(o), 3, 37, 0.0, 8.0)
    f_max = float(table.max())
    want, near = F.render(ubo, c, r, s, o, feature_rows(table.astype(np.float64), np.float64))
    sc = gsrt.Scene.from_model(ctx, c, r, s, o)
    sc.build_bvh()
    sc.set_features(table)
    rgba, feat = sc.render_features(ubo)
    sc.close()
    diff = np.abs(feat.astype(np.float64) - want[..., :3])
    kept = diff[~near]
    print(f"features vs f64, camera {cam}: {near.sum()} of {near.size} pixels float32-sensitive ({near.mean():.2%}); "
          f"L-inf all {diff.max():.3g}, without them {kept.max() if kept.size else 0.0:.3g}; bound {1e-3 * f_max:.3g}")
    assert want[..., 3].mean() > 0.1
    assert np.abs(rgba[..., 3].astype(np.float64) - want[..., 3]).max() <= 1e-3
    assert diff.max() <= 1e-3 * f_max


# ------------------------------------------------------------------------------------------------ 7: the API
def _d2h(ptr, shape):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros(shape, np.float32)
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def test_features_api(ctx):
    import torch

    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 5000, 21, True)
    n, C = len(o), 5
    table = noise(n, C, 41)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    W, H = 40, 24
    ubo = ubo_of(W, H, 4)
    plain, _ = sc.render(ubo, gsrt.MODE_COR)
    assert sc.features() == 0 and ctx.features_ptr() == 0
    with pytest.raises(gsrt.GsrtError) as e:  # no table yet
        sc.render_features(ubo)
    assert e.value.status == gsrt.E_STATE
    sc.set_features(table)
    assert sc.features() == C
    rgba, feat = sc.render_features(ubo)  # host pointers
    assert feat.shape == (H, W, C) and np.abs(feat).max() > 0
    assert ctx.features_ptr() != 0 and ctx.depth_ptr() == 0 and not ctx.slot_streams()
    assert _d2h(ctx.features_ptr(), (H, W, C)).tobytes() == feat.tobytes()
    assert _d2h(ctx.framebuffer_ptr, (H, W, 4)).tobytes() == rgba.tobytes()
    after, _ = sc.render(ubo, gsrt.MODE_COR)  # a plain frame after it: as the one before it
    assert after.tobytes() == plain.tobytes() and ctx.features_ptr() == 0
    sc.render_depth(ubo)
    assert ctx.depth_ptr() != 0 and ctx.features_ptr() == 0
    # a table given as a device pointer (padded on the device) is the same table
    d_table = torch.from_numpy(table).to("cuda:0")
    sc.set_features(d_table.data_ptr(), C)
    assert sc.render_features(ubo)[1].tobytes() == feat.tobytes()
    # device outputs
    d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_feat = torch.zeros((H, W, C), dtype=torch.float32, device="cuda:0")
    gsrt._check(gsrt.lib.gsrt_render_features(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0,
                                              ctypes.c_void_p(d_rgba.data_ptr()), ctypes.c_void_p(d_feat.data_ptr())), ctx)
    assert d_rgba.cpu().numpy().tobytes() == rgba.tobytes() and d_feat.cpu().numpy().tobytes() == feat.tobytes()
    # no outputs: the images stay in the ctx buffers; gsrt_render with the flag does the same
    sc.render(ubo, gsrt.MODE_COR)
    gsrt._check(gsrt.lib.gsrt_render_features(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0, None, None), ctx)
    assert _d2h(ctx.features_ptr(), (H, W, C)).tobytes() == feat.tobytes()
    sc.render(ubo, gsrt.MODE_COR)
    got, _ = sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURES)
    assert got.tobytes() == rgba.tobytes() and _d2h(ctx.features_ptr(), (H, W, C)).tobytes() == feat.tobytes()
    sc.render_async(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURES)
    ctx.synchronize()
    assert _d2h(ctx.features_ptr(), (H, W, C)).tobytes() == feat.tobytes()

    def refused(call, what, status=gsrt.E_ARG):
        with pytest.raises(gsrt.GsrtError) as e:
            call()
        assert e.value.status == status, what
        assert "FEATURES" in str(e.value) or "features" in str(e.value), (what, str(e.value))
        again, _ = sc.render(ubo, gsrt.MODE_COR)  # and the context renders as before
        assert again.tobytes() == plain.tobytes(), what

    refused(lambda: sc.render_features(ubo, gsrt.MODE_REF), "REF")
    refused(lambda: sc.render(ubo, gsrt.MODE_REF | gsrt.FLAG_FEATURES), "REF through gsrt_render")
    refused(lambda: sc.render_features(ubo, gsrt.MODE_COR | gsrt.FLAG_STATS), "STATS")
    refused(lambda: sc.render_features(ubo, gsrt.MODE_COR | gsrt.FLAG_OUT_DUMP8), "DUMP8")
    refused(lambda: sc.render_features(ubo, gsrt.MODE_COR | gsrt.FLAG_DEPTH), "DEPTH")
    refused(lambda: sc.render_depth(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURES), "DEPTH through render_depth")
    refused(lambda: sc.render_features_async(ubo, gsrt.MODE_COR | gsrt.FLAG_STATS), "STATS async")
    refused(lambda: sc.render_sharded_emulated(ubo, 2, gsrt.MODE_COR | gsrt.FLAG_FEATURES), "emulated shares")
    refused(lambda: sc.set_features(noise(n, 17, 1)), "17 channels")
    refused(lambda: sc.set_features(d_table.data_ptr(), 0), "0 channels with data")
    assert sc.features() == C and sc.render_features(ubo)[1].tobytes() == feat.tobytes()  # the table survived them

    # replacing the table between two queued frames changes the second frame only
    table2 = noise(n, 3, 43)
    d_a = torch.zeros((H, W, C), dtype=torch.float32, device="cuda:0")
    d_b = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    sc.render_features_async(ubo, d_feat=d_a.data_ptr())
    sc.set_features(table2)
    sc.render_features_async(ubo, d_feat=d_b.data_ptr())
    ctx.synchronize()
    feat2 = sc.render_features(ubo)[1]
    assert d_a.cpu().numpy().tobytes() == feat.tobytes() and d_b.cpu().numpy().tobytes() == feat2.tobytes()
    assert feat2.shape == (H, W, 3) and feat2.tobytes() != feat[..., :3].tobytes()

    # a removed table: E_STATE until there is one again
    sc.set_features(None)
    assert sc.features() == 0
    refused(lambda: sc.render_features(ubo), "table removed", gsrt.E_STATE)
    sc.set_features(table2)
    assert sc.render_features(ubo)[1].tobytes() == feat2.tobytes()

    # features are indexed by Gaussian id: an update of params and AABBs and a refit keep using the same table
    p, a = sc.download()
    d = np.random.default_rng(5).normal(0.0, 2e-2, (n, 3)).astype(np.float32)
    p1, a1 = p.copy(), a.copy()
    p1[:, :3] += d
    a1[:, :3] += d
    a1[:, 3:] += d
    sc.update(p1, a1)
    sc.refit_bvh()
    moved = sc.render_features(ubo)
    sc2 = gsrt.Scene.from_params(ctx, p1, a1, sh)
    sc2.build_bvh()
    sc2.set_features(table2)
    fresh = sc2.render_features(ubo)
    sc2.close()
    assert moved[0].tobytes() == fresh[0].tobytes() and moved[1].tobytes() == fresh[1].tobytes()
    assert moved[1].tobytes() != feat2.tobytes()

    sc.close()


def test_features_refused_on_sharded_frames():
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 5000, 21, True)
    with gsrt.Context(0) as cx:
        sc = gsrt.Scene.from_model(cx, c, r, s, o, sh)
        sc.build_bvh()
        sc.set_features(noise(len(o), 4, 47))
        ubo = ubo_of(40, 24, 4)
        plain, _ = sc.render(ubo, gsrt.MODE_COR)
        cx.comm_init_loopback()
        for call in (lambda: sc.render_sharded(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURES),
                     lambda: sc.render_sharded_async(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURES),
                     lambda: sc.render_sharded(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURES | gsrt.FLAG_OUT_DUMP8)):
            with pytest.raises(gsrt.GsrtError) as e:
                call()
            assert e.value.status == gsrt.E_ARG and "FEATURES" in str(e.value)
            assert sc.render_sharded(ubo, gsrt.MODE_COR).tobytes() == plain.tobytes()
            assert sc.render(ubo, gsrt.MODE_COR)[0].tobytes() == plain.tobytes()
        # whole frames on the same context still carry features
        rgba, feat = sc.render_features(ubo)
        assert np.abs(feat).max() > 0 and cx.features_ptr() != 0
        assert sc.render_sharded(ubo, gsrt.MODE_COR).tobytes() == plain.tobytes()
        assert cx.features_ptr() == 0


# ------------------------------------------------------------------------------------------------ 8: pipelined
@pytest.fixture(params=["adaptive", "0", "1"])
def slot_knob(request, monkeypatch):
    """the slot-stream choice of the plain frames: measured per frame, or forced off / on (GSRT_DEBUG_SLOT_STREAMS)"""
    if request.param != "adaptive":
        monkeypatch.setenv("GSRT_DEBUG_SLOT_STREAMS", request.param)
    return request.param


def test_pipelined_feature_frames_match_sync(ctx, slot_knob):
    """Eight feature frames interleaved with plain frames, queued without a sync in between, two cameras, device
    outputs, a scene update + refit in the middle: every frame's rgba and feature image equal its synchronous render.
    Feature frames take the in-order path whatever the plain frames around them choose."""
    import torch

    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 20000, 11, True)
    C = 7
    table = noise(len(o), C, 53)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    sc.set_features(table)
    p, a = sc.download()
    d = np.random.default_rng(5).normal(0.0, 2e-2, (len(p), 3)).astype(np.float32)
    p1, a1 = p.copy(), a.copy()
    p1[:, :3] += d
    a1[:, :3] += d
    a1[:, 3:] += d
    W, H, N = 64, 48, 16
    cams = [ubo_of(W, H, 4, gsrt.lookat((0.05, -0.03, 0.1), (0.02, 0, -1))),
            ubo_of(W, H, 4, gsrt.lookat((-0.2, 0.1, 0.3), (0.1, 0.05, -1)))]
    sc2 = gsrt.Scene.from_params(ctx, p1, a1, sh)
    sc2.build_bvh()
    sc2.set_features(table)
    want_f = {(g, k): scene.render_features(cams[k]) for g, scene in enumerate((sc, sc2)) for k in range(2)}
    want_p = {(g, k): scene.render(cams[k], gsrt.MODE_COR)[0] for g, scene in enumerate((sc, sc2)) for k in range(2)}
    sc2.close()
    is_feat = [i % 2 == 1 for i in range(N)]  # eight of the sixteen
    cam_of = [(i // 2) % 2 for i in range(N)]
    out = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(N)]
    fout = [torch.zeros((H, W, C), dtype=torch.float32, device="cuda:0") if is_feat[i] else None for i in range(N)]
    slots = []
    for i in range(N):
        if i == N // 2:
            sc.update(p1, a1)
            sc.refit_bvh()
        if is_feat[i]:
            sc.render_features_async(cams[cam_of[i]], d_rgba=out[i].data_ptr(), d_feat=fout[i].data_ptr())
            assert not ctx.slot_streams() and ctx.features_ptr() != 0 and ctx.depth_ptr() == 0
        else:
            sc.render_async(cams[cam_of[i]], gsrt.MODE_COR, d_rgba=out[i].data_ptr())
            assert ctx.features_ptr() == 0
            slots.append(ctx.slot_streams())
    ctx.synchronize()
    torch.cuda.synchronize()
    if slot_knob != "adaptive":  # plain frames around the feature frames keep their own choice
        assert all(slots) == (slot_knob == "1") and any(slots) == (slot_knob == "1")
    for i in range(N):
        key = (0 if i < N // 2 else 1, cam_of[i])
        if is_feat[i]:
            assert out[i].cpu().numpy().tobytes() == want_f[key][0].tobytes(), f"frame {i}: rgba differs"
            assert fout[i].cpu().numpy().tobytes() == want_f[key][1].tobytes(), f"frame {i}: features differ"
        else:
            assert out[i].cpu().numpy().tobytes() == want_p[key].tobytes(), f"frame {i}: rgba differs from its sync render"
    sc.close()
