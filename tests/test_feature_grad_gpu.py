"""Gradient frames (GSRT_FLAG_FEATURE_GRAD, gsrt_render_feature_grad): the backward of a feature frame to the feature
table, grad[g, c] = sum over the hits i of Gaussian g of w_i G[p, c] / ns.

The reference of every numeric check is the forward feature kernel, which tests/test_features_gpu.py ties to the oracle:
a feature frame of a one-hot table (16 Gaussians a frame, one per channel) gives W_g[p], Gaussian g's weight in pixel p,
exactly at 1 spp (a chain fma(1, w, F) keeps w), and grad_ref[g, c] = sum_p W_g[p] G[p, c] in float64.

The check that is independent of the forward kernel is tests/test_grad_f64_gpu.py (the float64 backward of
tests/cor_f64.py, on a scene where both clamps fire behind other hits); the references here cover what that one
cannot: float32 rounding bounds per entry, GSRT_FLAG_LUT frames and the API.
"""
import ctypes

import numpy as np
import pytest

import gsrt
import test_features_gpu as TF
from test_features_gpu import PLANES, _cloud, _d2h, noise, plane, synth_sh, u32, ubo_of

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
_W = {}


def weights_of(sc, ubo, mode=gsrt.MODE_COR):
    """W[g, y, x] (float32): Gaussian g's weight in each pixel of the scene's frame, from one-hot feature frames of the
    forward kernel, 16 Gaussians a frame; and the feature frame's rgba. Replaces the scene's feature table."""
    k, h, w = sc.n, int(ubo["height"][0]), int(ubo["width"][0])
    W = np.zeros((k, h, w), np.float32)
    for g0 in range(0, k, 16):
        m = min(16, k - g0)
        table = np.zeros((k, 16), np.float32)
        table[np.arange(g0, g0 + m), np.arange(m)] = 1.0
        sc.set_features(table)
        rgba, feat = sc.render_features(ubo, mode)
        W[g0:g0 + m] = np.moveaxis(feat[..., :m], 2, 0)
    return W, rgba


def weights(ctx, name, size, spp, lut=False):
    """weights_of the size x size frame of PLANES[name]. Computed once per case."""
    key = (name, size, spp, lut)
    if key not in _W:
        sc = gsrt.Scene.from_model(ctx, *plane(**PLANES[name]))
        try:
            sc.build_bvh()
            _W[key] = weights_of(sc, ubo_of(size, size, spp), gsrt.MODE_COR | (gsrt.FLAG_LUT if lut else 0))
        finally:
            sc.close()
    return _W[key]


def impulse_pixels(size):
    """16 pixels: the frame's and the 8x8 tiles' corners, the last row and column, and the centre, where rays of
    "stops" end inside a stage (asserted from the oracle's counts in test_impulses_one_sample_are_exact)"""
    e, h = size - 1, size // 2
    px = [(0, 0), (e, 0), (0, e), (e, e), (7, 7), (8, 8), (7, 8), (8, 7), (h + 1, h + 1), (h - 2, h), (h, h - 2), (h + 1, h - 1),
          (e, h), (h, e), (3, e), (e, 5)]
    assert len(set(px)) == 16
    return px


def impulses(size):
    G = np.zeros((size, size, 16), np.float32)
    vals = (np.float32(0.3) + np.float32(0.17) * np.arange(16, dtype=np.float32)).astype(np.float32)
    for c, (x, y) in enumerate(impulse_pixels(size)):
        G[y, x, c] = vals[c]
    return G, vals


# ------------------------------------------------------------------------------------------------ 1: impulses, 1 spp
@pytest.mark.parametrize("size", [16, 18])
@pytest.mark.parametrize("name", list(PLANES))
def test_impulses_one_sample_are_exact(ctx, name, size):
    """One non-zero of G per channel: every Gaussian receives at most one term per channel, so grad[g, c] has the bits
    of float32(W_g[p_c]) * float32(G[p_c, c]); Gaussians the pixel does not blend hold +0. With and without the LUT,
    scenes with and without SH rows; the framebuffer is the feature frame's RGBA byte for byte."""
    model = plane(**PLANES[name])
    k = len(model[3])
    ubo = ubo_of(size, size, 1)
    G, vals = impulses(size)
    if name == "stops":
        # some impulse pixel's ray stops inside a stage with candidates of that stage behind it (their masks lose the
        # lane: okg[c1] &= ~stopped), and its pixel leaves Gaussians unblended: one ray per pixel stops at list
        # position ncand - 1 (as tests/test_features_gpu.py reads the oracle's counts)
        _, st = TF.oracle_frame(model, None, size, size, 1)
        at = [st[y, x] for x, y in impulse_pixels(size)]
        assert any(s[3] == 1 and (s[0] - 1) % TF.K_GROUP != TF.K_GROUP - 1 and s[0] < k for s in at)
        W0 = weights(ctx, name, size, 1)[0]
        assert any(st[y, x, 3] == 1 and (W0[:, y, x] == 0).sum() == k - st[y, x, 1] > 0 for x, y in impulse_pixels(size))
    for lut in (False, True):
        W, rgba = weights(ctx, name, size, 1, lut)
        want = np.zeros((k, 16), np.float32)
        for c, (x, y) in enumerate(impulse_pixels(size)):
            want[:, c] = W[:, y, x] * vals[c]
        assert (want > 0).any()
        mode = gsrt.MODE_COR | (gsrt.FLAG_LUT if lut else 0)
        for with_sh in (False, True):
            sc = gsrt.Scene.from_model(ctx, *model, synth_sh(k) if with_sh else None)
            try:
                sc.build_bvh()
                got = sc.feature_grad(ubo, G, mode)
                fb = _d2h(ctx.framebuffer_ptr, (size, size, 4))
            finally:
                sc.close()
            label = f"{name} {size} lut {lut} sh {with_sh}"
            assert got.shape == (k, 16)
            assert np.array_equal(u32(got), u32(want)), label
            assert fb.tobytes() == rgba.tobytes(), label


# ------------------------------------------------------------------------------------------------ 2: impulses, 4 and 3 spp
@pytest.mark.parametrize("spp", [4, 3])
@pytest.mark.parametrize("size", [16, 18])
@pytest.mark.parametrize("name", list(PLANES))
def test_impulses_more_samples(ctx, name, size, spp):
    """The same G at 4 spp (samples in the wave) and 3 spp (passes): per entry within
    (ns + 8) 2^-23 W_g[p_c] |G[p_c, c]|: ns products and ns - 1 adds in any order, the forward's sample combination and
    division, the G / ns rounding, a factor 2 for second-order terms."""
    ubo = ubo_of(size, size, spp)
    assert (gsrt.tile_plan(ubo)["spp_lanes"] != spp) == (spp == 3)
    model = plane(**PLANES[name])
    G, vals = impulses(size)
    W, _ = weights(ctx, name, size, spp)
    sc = gsrt.Scene.from_model(ctx, *model)
    try:
        sc.build_bvh()
        got = sc.feature_grad(ubo, G).astype(np.float64)
    finally:
        sc.close()
    for c, (x, y) in enumerate(impulse_pixels(size)):
        ref = W[:, y, x].astype(np.float64) * float(vals[c])
        tol = (spp + 8) * EPS * np.abs(ref)
        assert (np.abs(got[:, c] - ref) <= tol).all(), (name, size, spp, c)
        assert not u32(got[:, c].astype(np.float32))[ref == 0].any()


# ------------------------------------------------------------------------------------------------ 3: dense random G
def dense_bound(W, G, ns):
    """grad_ref[g, c] and its bound (N_g + 8) 2^-23 sum_p W_g[p] |G[p, c]|, N_g = ns #{p : W_g[p] > 0}"""
    W64, G64 = W.astype(np.float64), G.astype(np.float64)
    ref = np.einsum("gyx,yxc->gc", W64, G64)
    ng = ns * (W > 0).sum(axis=(1, 2))
    return ref, (ng[:, None] + 8) * EPS * np.einsum("gyx,yxc->gc", W64, np.abs(G64))


@pytest.mark.parametrize("channels", [1, 5, 16])
@pytest.mark.parametrize("spp", [1, 4, 3])
@pytest.mark.parametrize("name", ["stops", "rounds", "past_group_list"])
def test_dense_gradient(ctx, name, spp, channels):
    size = 18
    ubo = ubo_of(size, size, spp)
    model = plane(**PLANES[name])
    G = noise(size * size, channels, 100 + channels).reshape(size, size, channels)
    W, _ = weights(ctx, name, size, spp)
    ref, bound = dense_bound(W, G, spp)
    sc = gsrt.Scene.from_model(ctx, *model)
    try:
        sc.build_bvh()
        got = sc.feature_grad(ubo, G).astype(np.float64)
    finally:
        sc.close()
    err = np.abs(got - ref)
    print(f"{name} spp {spp} C {channels}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.4f}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ 4: clouds
@pytest.mark.parametrize("cam", ["origin", "moved"])
@pytest.mark.parametrize("name", ["10k", "20k"])
def test_clouds_subset_sums_and_adjoint(ctx, name, cam):
    """16 seeded random subsets S_j of the Gaussians as an indicator table: sum_{g in S_j} grad[g, c] against
    sum_p feat_j[p] G[p, c], within (W H ns + n_max + 8) 2^-23 sum_p feat_j[p] |G[p, c]|; and the adjoint identity
    <G, render_features(f)> = <grad, f> for a random f with the two sides' bounds added."""
    model, sh, (w, h, spp) = _cloud(name)
    n = len(model[3])
    mv = TF.MV if cam == "origin" else gsrt.lookat((0.05, -0.03, 0.1), (0.02, 0, -1))
    ubo = ubo_of(w, h, spp, mv)
    rng = np.random.default_rng(77)
    ind = (rng.random((n, 16)) < 0.5).astype(np.float32)
    f = noise(n, 16, 79)
    G = noise(w * h, 16, 81).reshape(h, w, 16)
    _, st = TF.oracle_frame(model, None, w, h, spp, False, mv)
    n_max = int(st[..., 1].max())
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        sc.set_features(ind)
        feat_ind = sc.render_features(ubo)[1].astype(np.float64)
        sc.set_features(f)
        feat_f = sc.render_features(ubo)[1].astype(np.float64)
        sc.set_features(np.abs(f))
        feat_abs = sc.render_features(ubo)[1].astype(np.float64)
        grad = sc.feature_grad(ubo, G).astype(np.float64)
    finally:
        sc.close()
    G64 = G.astype(np.float64)
    k = (w * h * spp + n_max + 8) * EPS
    got = np.einsum("gj,gc->jc", ind.astype(np.float64), grad)
    ref = np.einsum("yxj,yxc->jc", feat_ind, G64)
    bound = k * np.einsum("yxj,yxc->jc", feat_ind, np.abs(G64))
    print(f"{name} {cam}: subsets worst error / bound = {(np.abs(got - ref) / bound).max():.4f}")
    assert (np.abs(got - ref) <= bound).all()
    lhs, rhs = (G64 * feat_f).sum(), (grad * f.astype(np.float64)).sum()
    both = 2 * k * (np.abs(G64) * feat_abs).sum()
    assert abs(lhs - rhs) <= both, (lhs, rhs, both)


# ------------------------------------------------------------------------------------------------ 5: masks, non-finite
def test_infinite_gradient_at_one_pixel_of_one(ctx):
    """G = +inf at one pixel of "one": the Gaussian reads +inf if that pixel blends it, and at a pixel it does not cover
    the gradient stays finite and equal to the run without it"""
    size = 18
    ubo = ubo_of(size, size, 1)
    W, _ = weights(ctx, "one", size, 1)
    G = noise(size * size, 2, 6).reshape(size, size, 2)
    inside = np.argwhere(W[0] > 0)
    outside = np.argwhere(W[0] == 0)
    assert len(inside) and len(outside)
    ref, bound = dense_bound(W, G, 1)
    sc = gsrt.Scene.from_model(ctx, *plane(**PLANES["one"]))
    try:
        sc.build_bvh()
        for (y, x), reaches in ((inside[len(inside) // 2], True), (outside[0], False)):
            Ginf = G.copy()
            Ginf[y, x, 1] = np.inf
            got = sc.feature_grad(ubo, Ginf)
            assert got.shape == (1, 2) and abs(float(got[0, 0]) - ref[0, 0]) <= bound[0, 0]
            if reaches:
                assert got[0, 1] == np.inf
            else:
                assert abs(float(got[0, 1]) - ref[0, 1]) <= bound[0, 1]
    finally:
        sc.close()


def test_masks_and_non_finite(ctx):
    """The same on "stops" (22 Gaussians: the pixel blends some and leaves others), G = 0, and the sentinels"""
    import torch

    size = 18
    ubo = ubo_of(size, size, 1)
    W, _ = weights(ctx, "stops", size, 1)
    model = plane(**PLANES["stops"])
    k = len(model[3])
    G = noise(size * size, 3, 5).reshape(size, size, 3)
    y, x = size // 2, size // 2 - 3
    hit = W[:, y, x] > 0
    assert hit.any() and not hit.all()
    Ginf = G.copy()
    Ginf[y, x, 1] = np.inf
    sc = gsrt.Scene.from_model(ctx, *model)
    try:
        sc.build_bvh()
        base = sc.feature_grad(ubo, G)
        got = sc.feature_grad(ubo, Ginf)
        assert (got[hit, 1] == np.inf).all() and np.isfinite(got[~hit]).all()
        assert np.isfinite(got[:, [0, 2]]).all()
        ref, bound = dense_bound(W, G, 1)
        assert (np.abs(got[~hit].astype(np.float64) - base[~hit]) <= 2 * bound[~hit]).all()
        assert (np.abs(got[:, [0, 2]].astype(np.float64) - base[:, [0, 2]]) <= 2 * bound[:, [0, 2]]).all()
        zero = sc.feature_grad(ubo, np.zeros((size, size, 3), np.float32))
        assert not u32(zero).any()  # all +0
        # a device table of n*C + 64 floats keeps its sentinels; accumulate == 0 overwrites sentinels in the table
        d_g = torch.from_numpy(G).to("cuda:0")
        d_t = torch.full((k * 3 + 64,), -7.5, dtype=torch.float32, device="cuda:0")
        sc.feature_grad_async(ubo, d_g.data_ptr(), 3, d_t.data_ptr())
        ctx.synchronize()
        t = d_t.cpu().numpy()
        assert (t[k * 3:] == -7.5).all()
        assert (np.abs(t[:k * 3].reshape(k, 3).astype(np.float64) - ref) <= bound).all()
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------ 6: accumulate
def test_accumulate_adds_frames(ctx):
    import torch

    model, sh, _ = _cloud("sh3_1k")
    n, C, w, h, spp = len(model[3]), 5, 48, 32, 4
    cams = [ubo_of(w, h, spp), ubo_of(w, h, spp, gsrt.lookat((0.05, -0.03, 0.1), (0.02, 0, -1)))]
    Gs = [noise(w * h, C, 31 + i).reshape(h, w, C) for i in range(2)]
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        refs = [dense_bound(weights_of(sc, cams[i])[0], Gs[i], spp) for i in range(2)]
        sc.set_features(None)
        parts = [sc.feature_grad(cams[i], Gs[i]).astype(np.float64) for i in range(2)]
        d_t = torch.full((n, C), 123.0, dtype=torch.float32, device="cuda:0")
        d_g = [torch.from_numpy(g).to("cuda:0") for g in Gs]
        sc.feature_grad_async(cams[0], d_g[0].data_ptr(), C, d_t.data_ptr(), accumulate=False)  # overwrites the sentinels
        sc.feature_grad_async(cams[1], d_g[1].data_ptr(), C, d_t.data_ptr(), accumulate=True)
        ctx.synchronize()
        got = d_t.cpu().numpy().astype(np.float64)
        # a host table cannot accumulate
        out = np.zeros((n, C), np.float32)
        st = gsrt.lib.gsrt_render_feature_grad(sc.handle, gsrt._p(cams[0]), gsrt.MODE_COR, 0, gsrt._p(Gs[0]), C,
                                               gsrt._p(out), 1)
        assert st == gsrt.E_ARG and "FEATURE_GRAD" in gsrt.lib.gsrt_last_error(ctx.handle).decode()
    finally:
        sc.close()
    # against the float64 sum of the two frames' references (one-hot feature frames of each camera): the two frames'
    # dense bounds added, plus one rounding of the sum; and against the float64 sum of the separate results
    for i in range(2):
        assert (np.abs(parts[i] - refs[i][0]) <= refs[i][1]).all()
    ref = refs[0][0] + refs[1][0]
    bound = refs[0][1] + refs[1][1] + EPS * np.abs(ref)
    print(f"accumulate: worst error / bound = {(np.abs(got - ref) / np.maximum(bound, 1e-300)).max():.4f}")
    assert (np.abs(got - ref) <= bound).all()
    assert (np.abs(got - (parts[0] + parts[1])) <= 2 * bound).all()
    assert np.abs(refs[1][0]).max() > 0


# ------------------------------------------------------------------------------------------------ 7: API and ordering
def test_feature_grad_api(ctx):
    import torch

    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 2000, 21, True)
    n, C, W, H, spp = len(o), 5, 40, 24, 4
    ubo = ubo_of(W, H, spp)
    G = noise(W * H, C, 61).reshape(H, W, C)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    plain, _ = sc.render(ubo, gsrt.MODE_COR)
    Wg, frgba = weights_of(sc, ubo)  # the reference: one-hot feature frames of this scene
    ref, bound = dense_bound(Wg, G, spp)
    tol = 2 * bound  # two device results, each within the bound of the reference
    sc.set_features(None)  # no feature table is needed
    grad = sc.feature_grad(ubo, G)  # host in, host out
    assert grad.shape == (n, C) and np.abs(grad).max() > 0
    assert (np.abs(grad.astype(np.float64) - ref) <= bound).all()
    assert ctx.features_ptr() == 0 and ctx.depth_ptr() == 0 and not ctx.slot_streams()
    assert _d2h(ctx.framebuffer_ptr, (H, W, 4)).tobytes() == frgba.tobytes()
    assert sc.render(ubo, gsrt.MODE_COR)[0].tobytes() == plain.tobytes()
    one = sc.feature_grad(ubo, G[..., 0])  # (H, W): one channel
    assert one.shape == (n, 1) and (np.abs(one[:, 0].astype(np.float64) - ref[:, 0]) <= bound[:, 0]).all()
    # device in and out through the blocking call, and mixed
    d_g = torch.from_numpy(G).to("cuda:0")
    d_t = torch.zeros((n, C), dtype=torch.float32, device="cuda:0")
    gsrt._check(gsrt.lib.gsrt_render_feature_grad(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0, ctypes.c_void_p(d_g.data_ptr()),
                                                  C, ctypes.c_void_p(d_t.data_ptr()), 0), ctx)
    assert (np.abs(d_t.cpu().numpy().astype(np.float64) - ref) <= bound).all()
    out = np.zeros((n, C), np.float32)
    gsrt._check(gsrt.lib.gsrt_render_feature_grad(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0, ctypes.c_void_p(d_g.data_ptr()),
                                                  C, gsrt._p(out), 0), ctx)
    assert (np.abs(out.astype(np.float64) - ref) <= bound).all()
    d_t.fill_(-3.0)  # host image, device table, written (accumulate == 0)
    gsrt._check(gsrt.lib.gsrt_render_feature_grad(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0, gsrt._p(G), C,
                                                  ctypes.c_void_p(d_t.data_ptr()), 0), ctx)
    assert (np.abs(d_t.cpu().numpy().astype(np.float64) - ref) <= bound).all()
    # contributions: feature_grad of ones, and its sum over g is the frame's sum of w, within the summed bounds
    contrib = sc.contributions(ubo)
    ones = sc.feature_grad(ubo, np.ones((H, W), np.float32))[:, 0]
    cref, cbound = dense_bound(Wg, np.ones((H, W, 1), np.float32), spp)
    assert contrib.shape == (n,)
    assert (np.abs(contrib.astype(np.float64) - cref[:, 0]) <= cbound[:, 0]).all()
    assert (np.abs(ones.astype(np.float64) - cref[:, 0]) <= cbound[:, 0]).all()
    total = float(frgba[..., 0].astype(np.float64).sum())
    print(f"contributions: sum {contrib.astype(np.float64).sum():.6f}, frame {total:.6f}, bound {cbound.sum():.3g}")
    assert abs(float(contrib.astype(np.float64).sum()) - total) <= cbound.sum()

    def refused(call, what):
        with pytest.raises(gsrt.GsrtError) as e:
            call()
        assert e.value.status == gsrt.E_ARG, what
        assert "FEATURE_GRAD" in str(e.value), (what, str(e.value))
        assert sc.render(ubo, gsrt.MODE_COR)[0].tobytes() == plain.tobytes(), what

    def raw(mode, g=G, ch=C, table=out):
        gsrt._check(gsrt.lib.gsrt_render_feature_grad(sc.handle, gsrt._p(ubo), mode, 0, gsrt._p(g) if g is not None else None,
                                                      ch, gsrt._p(table) if table is not None else None, 0), ctx)

    refused(lambda: sc.feature_grad(ubo, G, gsrt.MODE_REF), "REF")
    refused(lambda: sc.feature_grad(ubo, G, gsrt.MODE_COR | gsrt.FLAG_STATS), "STATS")
    refused(lambda: sc.feature_grad(ubo, G, gsrt.MODE_COR | gsrt.FLAG_OUT_DUMP8), "DUMP8")
    refused(lambda: sc.feature_grad(ubo, G, gsrt.MODE_COR | gsrt.FLAG_DEPTH), "DEPTH")
    refused(lambda: sc.feature_grad(ubo, G, gsrt.MODE_COR | gsrt.FLAG_FEATURES), "FEATURES")
    refused(lambda: sc.feature_grad_async(ubo, d_g.data_ptr(), C, d_t.data_ptr(), mode=gsrt.MODE_COR | gsrt.FLAG_STATS), "async")
    refused(lambda: sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURE_GRAD), "gsrt_render")
    refused(lambda: sc.render_async(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURE_GRAD), "gsrt_render_async")
    refused(lambda: sc.render_depth(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURE_GRAD), "render_depth")
    refused(lambda: sc.render_sharded_emulated(ubo, 2, gsrt.MODE_COR | gsrt.FLAG_FEATURE_GRAD), "emulated shares")
    refused(lambda: raw(gsrt.MODE_COR, ch=0), "0 channels")
    refused(lambda: raw(gsrt.MODE_COR, ch=17), "17 channels")
    refused(lambda: raw(gsrt.MODE_COR, g=None), "NULL image")
    refused(lambda: raw(gsrt.MODE_COR, table=None), "NULL table")
    # a scene with a mesh
    scm = gsrt.Scene.from_model(ctx, c[:100], r[:100], s[:100], o[:100])
    v, ix = gsrt.sphere_mesh((0.0, 0.0, -3.0), 0.5)
    scm.add_mesh(v, ix)
    scm.build_bvh()
    with pytest.raises(gsrt.GsrtError) as e:
        scm.feature_grad(ubo, G)
    assert e.value.status == gsrt.E_ARG and "FEATURE_GRAD" in str(e.value)
    scm.close()
    assert (np.abs(sc.feature_grad(ubo, G).astype(np.float64) - ref) <= bound).all()  # and gradients as before

    # an update + refit between two queued gradient frames changes the second only
    p, a = sc.download()
    d = np.random.default_rng(5).normal(0.0, 2e-2, (n, 3)).astype(np.float32)
    p1, a1 = p.copy(), a.copy()
    p1[:, :3] += d
    a1[:, :3] += d
    a1[:, 3:] += d
    d_a = torch.zeros((n, C), dtype=torch.float32, device="cuda:0")
    d_b = torch.zeros((n, C), dtype=torch.float32, device="cuda:0")
    sc.feature_grad_async(ubo, d_g.data_ptr(), C, d_a.data_ptr())
    sc.update(p1, a1)
    sc.refit_bvh()
    sc.feature_grad_async(ubo, d_g.data_ptr(), C, d_b.data_ptr())
    ctx.synchronize()
    ref1, bound1 = dense_bound(weights_of(sc, ubo)[0], G, spp)  # the moved scene's own reference
    assert (np.abs(d_a.cpu().numpy().astype(np.float64) - ref) <= bound).all()
    assert (np.abs(d_b.cpu().numpy().astype(np.float64) - ref1) <= bound1).all()
    assert np.abs(ref1 - ref).max() > 10 * max(bound.max(), bound1.max())
    sc.close()


def test_feature_grad_refused_on_sharded_frames():
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 5000, 21, True)
    with gsrt.Context(0) as cx:
        sc = gsrt.Scene.from_model(cx, c, r, s, o, sh)
        sc.build_bvh()
        ubo = ubo_of(40, 24, 4)
        plain, _ = sc.render(ubo, gsrt.MODE_COR)
        cx.comm_init_loopback()
        for call in (lambda: sc.render_sharded(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURE_GRAD),
                     lambda: sc.render_sharded_async(ubo, gsrt.MODE_COR | gsrt.FLAG_FEATURE_GRAD)):
            with pytest.raises(gsrt.GsrtError) as e:
                call()
            assert e.value.status == gsrt.E_ARG and "FEATURE_GRAD" in str(e.value)
            assert sc.render_sharded(ubo, gsrt.MODE_COR).tobytes() == plain.tobytes()


@pytest.fixture(params=["adaptive", "0", "1"])
def slot_knob(request, monkeypatch):
    if request.param != "adaptive":
        monkeypatch.setenv("GSRT_DEBUG_SLOT_STREAMS", request.param)
    return request.param


def test_frames_around_gradient_frames_match_sync(ctx, slot_knob):
    """Plain, depth and feature frames queued before and after gradient frames, without a sync in between, are
    byte-identical to their synchronous renders, whatever the plain frames' slot-stream choice."""
    import torch

    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 20000, 11, True)
    n, C, W, H = len(o), 7, 64, 48
    ubo = ubo_of(W, H, 4, gsrt.lookat((0.05, -0.03, 0.1), (0.02, 0, -1)))
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    sc.set_features(noise(n, C, 53))
    want_p = sc.render(ubo, gsrt.MODE_COR)[0]
    want_d = sc.render_depth(ubo)
    want_f = sc.render_features(ubo)
    d_g = torch.from_numpy(noise(W * H, C, 3).reshape(H, W, C)).to("cuda:0")
    d_t = torch.zeros((n, C), dtype=torch.float32, device="cuda:0")
    kinds = ["plain", "grad", "plain", "depth", "grad", "feat", "grad", "plain", "plain", "grad", "feat", "depth"]
    out = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in kinds]
    aux = [torch.zeros((H, W, C if kd == "feat" else 1), dtype=torch.float32, device="cuda:0") for kd in kinds]
    for i, kd in enumerate(kinds):
        if kd == "plain":
            sc.render_async(ubo, gsrt.MODE_COR, d_rgba=out[i].data_ptr())
        elif kd == "depth":
            sc.render_depth_async(ubo, d_rgba=out[i].data_ptr(), d_depth=aux[i].data_ptr())
        elif kd == "feat":
            sc.render_features_async(ubo, d_rgba=out[i].data_ptr(), d_feat=aux[i].data_ptr())
        else:
            sc.feature_grad_async(ubo, d_g.data_ptr(), C, d_t.data_ptr(), accumulate=True)
            assert not ctx.slot_streams() and ctx.features_ptr() == 0 and ctx.depth_ptr() == 0
    ctx.synchronize()
    torch.cuda.synchronize()
    for i, kd in enumerate(kinds):
        if kd == "plain":
            assert out[i].cpu().numpy().tobytes() == want_p.tobytes(), i
        elif kd == "depth":
            assert out[i].cpu().numpy().tobytes() == want_d[0].tobytes(), i
            assert aux[i].cpu().numpy()[..., 0].tobytes() == want_d[1].tobytes(), i
        elif kd == "feat":
            assert out[i].cpu().numpy().tobytes() == want_f[0].tobytes() and aux[i].cpu().numpy().tobytes() == want_f[1].tobytes(), i
    assert np.abs(d_t.cpu().numpy()).max() > 0
    sc.close()


# ------------------------------------------------------------------------------------------------ 8: autograd
def test_autograd_descends_and_matches_feature_grad(ctx):
    """20 steps of plain gradient descent on a 3-channel table against a target rendered from a known table: the loss
    0.5 |render(t) - target|^2 strictly decreases at the step 1 / max_g (sum_p W_g[p]) ... of a Jacobi preconditioner:
    the Hessian A^T A has row sums sum_p W_g[p] sum_g' W_g'[p] <= contributions[g] (sum_g' W_g'[p] = 1 - T <= 1), so
    its largest eigenvalue is at most max_g contributions[g], and any step below 2 / that decreases the loss. The
    backward's output is Scene.feature_grad of the same upstream gradient: both lie within the dense bound of the
    reference built from one-hot feature frames."""
    import torch

    from gsrt.autograd import render_features

    model, sh, _ = _cloud("sh3_1k")
    n, C, w, h, spp = len(model[3]), 3, 48, 32, 4
    ubo = ubo_of(w, h, spp)
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        Wg, _ = weights_of(sc, ubo)
        contrib = sc.contributions(ubo)
        assert contrib.max() > 0
        step = 1.0 / float(contrib.max())
        known = torch.from_numpy(noise(n, C, 91)).to("cuda:0")
        with torch.no_grad():
            target = render_features(sc, ubo, known)[1].clone()
        table = torch.zeros((n, C), dtype=torch.float32, device="cuda:0", requires_grad=True)
        losses = []
        for it in range(20):
            rgba, feat = render_features(sc, ubo, table)
            assert not rgba.requires_grad
            loss = 0.5 * ((feat - target).double() ** 2).sum()
            losses.append(float(loss.detach()))
            table.grad = None
            loss.backward()
            if it == 0:
                Gup = (feat - target).detach().cpu().numpy()
                direct = sc.feature_grad(ubo, Gup).astype(np.float64)
                ref, bound = dense_bound(Wg, Gup, spp)
                back = table.grad.cpu().numpy().astype(np.float64)
                assert (np.abs(back - ref) <= bound).all() and (np.abs(direct - ref) <= bound).all()
                assert (np.abs(back - direct) <= 2 * bound).all()
            with torch.no_grad():
                table -= step * table.grad
        assert all(b < a for a, b in zip(losses, losses[1:])), losses
        assert losses[-1] < 0.9 * losses[0]
    finally:
        sc.close()
