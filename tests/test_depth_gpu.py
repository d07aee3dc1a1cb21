"""The expected-depth output of COR frames (GSRT_FLAG_DEPTH, include/gsrt.h): depth = sum of z w over each ray's blended
hits, z the float32 view depth of the Gaussian's centre, w = alpha T the colour blend's own weight, combined over a
pixel's samples exactly as the colour is.

References, none of which needed a change to the oracle:
  * a depth plane: every z is exactly 4, so depth must equal 4 x (the red channel of the same geometry rendered without
    SH rows, where colour is 1 and red = sum w), bit for bit: a power-of-two scale commutes with every rounding of the
    chain (the fma per hit, the pairwise tree over in-wave samples, the running sum over passes, the division);
  * the oracle's colour path carrying depth: SH rows with s_k = 0 for k >= 1 and s_0 = (z - 0.5) / Y0 in all three
    channels make the colour fl(fl(s_0 Y0) + 0.5) ~ z, so the oracle's red channel is sum w z with the blend's own
    decisions;
  * tests/cor_f64.py, the independent float64 restatement, given the same rows in float64.

Every frame here is at most 64x48 pixels over at most 20k Gaussians.
"""
import ctypes

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


def depth_rows(z, dtype=np.float32):
    """SH rows whose colour is (an encoding of) z in every channel, whatever the ray direction"""
    sh = np.zeros((len(z), 16, 3), dtype)
    sh[:, 0, :] = ((np.asarray(z, dtype) - dtype(0.5)) / dtype(Y0))[:, None]
    return sh


def encoding_cost(z):
    """the largest |fl(fl(s0 Y0) + 0.5) - z| over the Gaussians, in float32: what the rows' encoding of z costs"""
    s0 = depth_rows(z)[:, 0, 0]
    enc = (s0 * Y0).astype(np.float32) + np.float32(0.5)
    return float(np.abs(enc.astype(np.float64) - z.astype(np.float64)).max())


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


def oracle_frame(model, sh, w, h, spp, lut=False):
    p, a = O.gauss_from_model(*model)
    ref = O.render(p, a, O.make_ubo(MV, FOV, w, h, 1.0, spp, 16), O.MODE_COR | (O.FLAG_LUT if lut else 0), sh=sh,
                   bvh=O.Bvh(a), want_stats=True, threads=4)
    return ref["rgba"], ref["stats"].astype(np.int64)


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1 + 2: the plane
@pytest.mark.parametrize("spp", [1, 4, 3])
@pytest.mark.parametrize("size", [16, 18])
@pytest.mark.parametrize("name", list(PLANES))
def test_depth_plane_is_exact(ctx, name, size, spp):
    """Every centre at view depth exactly 4: depth == 4 x (sum w), bit for bit, for SH and no-SH scenes with and without
    the LUT (the four DEPTH instantiations of k_render_cor), through stops inside a stage, continuation rounds, the
    group list's end and, at 3 spp, the multi-pass path; the depth frame's rgba is the plain frame's and the oracle's."""
    model = plane(**PLANES[name])
    k = len(model[3])
    assert np.array_equal(np.asarray(MV, np.float32).reshape(4, 4), np.eye(4, dtype=np.float32))
    assert (model[0][:, 2] == np.float32(-4.0)).all()  # with the identity modelview every z_i is exactly 4.0f
    ubo = ubo_of(size, size, spp)
    pl = gsrt.tile_plan(ubo)
    assert (pl["spp_lanes"] != spp) == (spp == 3)  # 3 spp run as passes, 1 and 4 in the wave
    sum_w = {}
    for with_sh in (False, True):
        sh = synth_sh(k) if with_sh else None
        sc = gsrt.Scene.from_model(ctx, *model, sh)
        try:
            sc.build_bvh()
            for lut in (False, True):
                mode = gsrt.MODE_COR | (gsrt.FLAG_LUT if lut else 0)
                label = f"{name} {size}x{size} spp {spp} sh {with_sh} lut {lut}"
                plain, _ = sc.render(ubo, mode)
                rgba, depth = sc.render_depth(ubo, mode)
                want, st = oracle_frame(model, sh, size, size, spp, lut)
                assert rgba.tobytes() == plain.tobytes(), label
                assert rgba.tobytes() == want.tobytes(), label
                if not with_sh:
                    sum_w[lut] = rgba[..., 0].copy()  # colour 1: red = sum w
                    # the scene still does what it is here for
                    nblend, nstop = st[..., 1], st[..., 3]
                    if name == "one":
                        assert (rgba[..., 3] == 0).any() and (rgba[..., 3] > 0).any()
                    elif name == "stops":
                        assert nstop.max() > 0
                        if spp == 1:  # one ray per pixel: a stop at list position ncand - 1
                            pos = (st[..., 0] - 1)[nstop == 1]
                            assert set((pos % K_GROUP).tolist()) == {0, 1, 2, 3}
                    elif name == "rounds":
                        assert nblend.min() > K_CAP * spp
                    else:
                        assert nblend.min() > K_GLIST * spp
                assert np.array_equal(u32(depth), u32(np.float32(4.0) * sum_w[lut])), label
                assert not u32(depth)[rgba[..., 3] == 0].any(), label  # no blend: exactly +0
        finally:
            sc.close()


# ------------------------------------------------------------------------------------------------ 3 + 4: clouds
def _cloud(name):
    if name == "sh3_1k":
        import os
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cor_sh3_1k.npz"))
        return (z["center"], z["rot"], z["scale"], z["opacity"]), z["sh"], (48, 32, 4)
    if name == "10k":
        c, r, s, o, _ = gsrt.synth_cloud(gsrt.SYNTH_COR, 10000, 42, False)
        return (c, r, s, o), None, (64, 48, 1)
    c, r, s, o, _ = gsrt.synth_cloud(gsrt.SYNTH_COR, 20000, 7, False)
    return (c, r, s, o), None, (64, 48, 3)


@pytest.mark.parametrize("name", ["sh3_1k", "10k", "20k"])
def test_depth_of_clouds_matches_the_oracle(ctx, name):
    """General clouds under the origin camera (z = -c_z exactly) against the oracle's depth-coloured frame. Tolerance
    from the reference side only: tol = delta + 2 n_max 2^-24 z_max, delta the rows' encoding cost, n_max the oracle's
    largest per-pixel blend count (one fma rounding per hit in each of the two chains). Every pixel is asserted."""
    model, sh_own, (w, h, spp) = _cloud(name)
    model = tuple(np.ascontiguousarray(a, np.float32) for a in model)
    z = -model[0][:, 2]
    rows = depth_rows(z)
    ubo = ubo_of(w, h, spp)
    want, st = oracle_frame(model, rows, w, h, spp)
    z_max = float(z[z > 0].max())
    tol = encoding_cost(z) + 2.0 * float(st[..., 1].max()) * 2.0 ** -24 * z_max
    sc = gsrt.Scene.from_model(ctx, *model, rows)
    sc.build_bvh()
    plain, _ = sc.render(ubo, gsrt.MODE_COR)
    rgba, depth = sc.render_depth(ubo, gsrt.MODE_COR)
    sc.close()
    assert rgba.tobytes() == plain.tobytes() and rgba.tobytes() == want.tobytes()
    linf = float(np.abs(depth.astype(np.float64) - want[..., 0].astype(np.float64)).max())
    print(f"{name}: depth vs oracle L-inf {linf:.3g}, tol {tol:.3g} (n_max {st[..., 1].max()}, z_max {z_max:.4g})")
    assert (rgba[..., 3] > 0).mean() > 0.5 and depth.max() > 1.0
    assert linf <= tol
    # the scene with its own colours (SH-3 rows, or none: the no-SH kernel) blends the same hits: the same depth bits
    sc = gsrt.Scene.from_model(ctx, *model, sh_own)
    sc.build_bvh()
    plain, _ = sc.render(ubo, gsrt.MODE_COR)
    rgba2, depth2 = sc.render_depth(ubo, gsrt.MODE_COR)
    sc.close()
    assert rgba2.tobytes() == plain.tobytes()
    assert np.array_equal(u32(depth2), u32(depth))
    assert np.array_equal(u32(rgba2[..., 3]), u32(rgba[..., 3]))


@pytest.mark.parametrize("cam", ["origin", "moved"])
def test_depth_matches_f64(ctx, cam):
    """Against the independent float64 restatement given the depth rows in float64: L-inf <= 1e-3 z_max on every pixel
    (the project's 1e-3 criterion applied to depth / z_max); the float32-sensitive share is reported, not excluded."""
    (c, r, s, o), _, (w, h, spp) = _cloud("10k")
    mv = MV if cam == "origin" else gsrt.lookat((0.3, -0.2, 0.5), (0.1, 0.05, -1.0))
    ubo = ubo_of(w, h, spp, mv)
    u = F.Ubo(ubo)
    z64 = -(np.concatenate([c.astype(np.float64), np.ones((len(c), 1))], 1) @ u.MV.T)[:, 2]
    want, near = F.render(ubo, c, r, s, o, depth_rows(z64, np.float64))
    z_max = float(z64[z64 > 0].max())
    sc = gsrt.Scene.from_model(ctx, c, r, s, o)
    sc.build_bvh()
    rgba, depth = sc.render_depth(ubo, gsrt.MODE_COR)
    sc.close()
    diff = np.abs(depth.astype(np.float64) - want[..., 0])
    kept = diff[~near]
    print(f"depth vs f64, camera {cam}: {near.sum()} of {near.size} pixels float32-sensitive ({near.mean():.2%}); "
          f"L-inf all {diff.max():.3g}, without them {kept.max() if kept.size else 0.0:.3g}; bound {1e-3 * z_max:.3g}")
    assert want[..., 3].mean() > 0.1
    assert np.abs(rgba[..., 3].astype(np.float64) - want[..., 3]).max() <= 1e-3
    assert diff.max() <= 1e-3 * z_max


# ------------------------------------------------------------------------------------------------ 5: the API
def _d2h(ptr, shape):
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.zeros(shape, np.float32)
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def test_depth_api(ctx):
    import torch

    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 5000, 21, True)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    W, H = 40, 24
    ubo = ubo_of(W, H, 4)
    plain, _ = sc.render(ubo, gsrt.MODE_COR)
    assert ctx.depth_ptr() == 0  # a plain frame leaves no depth image
    rgba, depth = sc.render_depth(ubo)  # host pointers
    assert rgba.tobytes() == plain.tobytes() and depth.max() > 0
    assert ctx.depth_ptr() != 0 and not ctx.slot_streams()
    assert _d2h(ctx.depth_ptr(), (H, W)).tobytes() == depth.tobytes()
    # device pointers
    d_rgba = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_depth = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    gsrt._check(gsrt.lib.gsrt_render_depth(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0, ctypes.c_void_p(d_rgba.data_ptr()),
                                           ctypes.c_void_p(d_depth.data_ptr())), ctx)
    assert d_rgba.cpu().numpy().tobytes() == plain.tobytes() and d_depth.cpu().numpy().tobytes() == depth.tobytes()
    # no outputs: the images stay in the ctx buffers; gsrt_render with the flag does the same
    sc.render(ubo, gsrt.MODE_COR)
    assert ctx.depth_ptr() == 0
    gsrt._check(gsrt.lib.gsrt_render_depth(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0, None, None), ctx)
    assert _d2h(ctx.depth_ptr(), (H, W)).tobytes() == depth.tobytes()
    assert _d2h(ctx.framebuffer_ptr, (H, W, 4)).tobytes() == plain.tobytes()
    sc.render(ubo, gsrt.MODE_COR)
    got, _ = sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_DEPTH)
    assert got.tobytes() == plain.tobytes() and _d2h(ctx.depth_ptr(), (H, W)).tobytes() == depth.tobytes()
    sc.render_async(ubo, gsrt.MODE_COR)
    ctx.synchronize()
    assert ctx.depth_ptr() == 0
    sc.render_depth_async(ubo, d_depth=d_depth.zero_().data_ptr())
    ctx.synchronize()
    assert d_depth.cpu().numpy().tobytes() == depth.tobytes()

    def refused(call, what):
        with pytest.raises(gsrt.GsrtError) as e:
            call()
        assert e.value.status == gsrt.E_ARG, what
        assert "DEPTH" in str(e.value) or "bad mode" in str(e.value), (what, str(e.value))
        again, _ = sc.render(ubo, gsrt.MODE_COR)  # and the context renders as before
        assert again.tobytes() == plain.tobytes(), what

    refused(lambda: sc.render_depth(ubo, gsrt.MODE_REF), "REF")
    refused(lambda: sc.render(ubo, gsrt.MODE_REF | gsrt.FLAG_DEPTH), "REF through gsrt_render")
    refused(lambda: sc.render_depth(ubo, gsrt.MODE_COR | gsrt.FLAG_STATS), "STATS")
    refused(lambda: sc.render_depth(ubo, gsrt.MODE_COR | gsrt.FLAG_OUT_DUMP8), "DUMP8")
    refused(lambda: sc.render_depth_async(ubo, gsrt.MODE_COR | gsrt.FLAG_STATS), "STATS async")
    refused(lambda: sc.render_sharded_emulated(ubo, 2, gsrt.MODE_COR | gsrt.FLAG_DEPTH), "emulated shares")
    sc.close()


def test_depth_refused_on_sharded_frames():
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 5000, 21, True)
    with gsrt.Context(0) as cx:
        sc = gsrt.Scene.from_model(cx, c, r, s, o, sh)
        sc.build_bvh()
        ubo = ubo_of(40, 24, 4)
        plain, _ = sc.render(ubo, gsrt.MODE_COR)
        cx.comm_init_loopback()
        for call in (lambda: sc.render_sharded(ubo, gsrt.MODE_COR | gsrt.FLAG_DEPTH),
                     lambda: sc.render_sharded_async(ubo, gsrt.MODE_COR | gsrt.FLAG_DEPTH),
                     lambda: sc.render_sharded(ubo, gsrt.MODE_COR | gsrt.FLAG_DEPTH | gsrt.FLAG_OUT_DUMP8)):
            with pytest.raises(gsrt.GsrtError) as e:
                call()
            assert e.value.status == gsrt.E_ARG and "DEPTH" in str(e.value)
            assert sc.render_sharded(ubo, gsrt.MODE_COR).tobytes() == plain.tobytes()
            assert sc.render(ubo, gsrt.MODE_COR)[0].tobytes() == plain.tobytes()
        # whole frames on the same context still carry depth
        rgba, depth = sc.render_depth(ubo)
        assert rgba.tobytes() == plain.tobytes() and depth.max() > 0
        assert sc.render_sharded(ubo, gsrt.MODE_COR).tobytes() == plain.tobytes()
        assert cx.depth_ptr() == 0


# ------------------------------------------------------------------------------------------------ 6: pipelined
@pytest.fixture(params=["adaptive", "0", "1"])
def slot_knob(request, monkeypatch):
    """the slot-stream choice of the plain frames: measured per frame, or forced off / on (GSRT_DEBUG_SLOT_STREAMS)"""
    if request.param != "adaptive":
        monkeypatch.setenv("GSRT_DEBUG_SLOT_STREAMS", request.param)
    return request.param


def test_pipelined_depth_frames_match_sync(ctx, slot_knob):
    """Twelve frames queued without a sync in between (plain, depth, plain, plain, depth, ...), two cameras, device
    outputs, a scene update + refit in the middle: every frame's rgba and depth equal its synchronous render. Depth
    frames take the in-order path whatever the plain frames around them choose."""
    import torch

    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 20000, 11, True)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    p, a = sc.download()
    d = np.random.default_rng(5).normal(0.0, 2e-2, (len(p), 3)).astype(np.float32)
    p1, a1 = p.copy(), a.copy()
    p1[:, :3] += d
    a1[:, :3] += d
    a1[:, 3:] += d
    W, H, N = 64, 48, 12
    cams = [ubo_of(W, H, 4, gsrt.lookat((0.05, -0.03, 0.1), (0.02, 0, -1))),
            ubo_of(W, H, 4, gsrt.lookat((-0.2, 0.1, 0.3), (0.1, 0.05, -1)))]
    sc2 = gsrt.Scene.from_params(ctx, p1, a1, sh)
    sc2.build_bvh()
    want = {(g, k): scene.render_depth(cams[k]) for g, scene in enumerate((sc, sc2)) for k in range(2)}
    for (g, k), (w_rgba, _) in want.items():
        assert (sc, sc2)[g].render(cams[k], gsrt.MODE_COR)[0].tobytes() == w_rgba.tobytes()
    sc2.close()
    is_depth = [i % 3 == 1 for i in range(N)]
    out = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(N)]
    dout = [torch.zeros((H, W), dtype=torch.float32, device="cuda:0") if is_depth[i] else None for i in range(N)]
    slots = []
    for i in range(N):
        if i == N // 2:
            sc.update(p1, a1)
            sc.refit_bvh()
        if is_depth[i]:
            sc.render_depth_async(cams[i % 2], d_rgba=out[i].data_ptr(), d_depth=dout[i].data_ptr())
            assert not ctx.slot_streams() and ctx.depth_ptr() != 0
        else:
            sc.render_async(cams[i % 2], gsrt.MODE_COR, d_rgba=out[i].data_ptr())
            assert ctx.depth_ptr() == 0
            slots.append(ctx.slot_streams())
    ctx.synchronize()
    torch.cuda.synchronize()
    if slot_knob != "adaptive":  # plain frames around the depth frames keep their own choice
        assert all(slots) == (slot_knob == "1") and any(slots) == (slot_knob == "1")
    for i in range(N):
        w_rgba, w_depth = want[(0 if i < N // 2 else 1, i % 2)]
        assert out[i].cpu().numpy().tobytes() == w_rgba.tobytes(), f"frame {i}: rgba differs from its synchronous render"
        if is_depth[i]:
            assert dout[i].cpu().numpy().tobytes() == w_depth.tobytes(), f"frame {i}: depth differs"
    sc.close()
