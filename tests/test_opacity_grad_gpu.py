"""Opacity gradient frames (GSRT_FLAG_OPACITY_GRAD, gsrt_render_opacity_grad): the backward of a COR colour frame (RGBA)
to each Gaussian's opacity, grad[g] = sum over the unclamped hits i of Gaussian g of d_i e_i (the definition: gsrt.h).

The reference is built only from forward kernels that existing tests tie to the oracle:
  * W[s, g, p], Gaussian g's float32 weight in sample s of pixel p, from one-hot feature frames (sample_weights);
  * the hits of a ray are the g with W > 0, ordered by (float32 view depth, id), the key order; the view depth is
    -(((z0 x + z1 y) + z2 z) + z3) in float32, the kernel's own expression (mul4v), exactly -c_z under the origin camera;
  * in float64, with T_1 = 1: alpha_i = w_i / T_i, T_{i+1} = T_i - w_i, e_i = alpha_i / o_g;
  * col: 1 without SH rows; fl(fl(s0 Y0) + 0.5) for tables with coefficient 0 only (feature_rows);
    0.5 + Y0 s_0 + sum_{q >= 1} B[s, q, p] sh[g, q, ch] with the kernel's basis B (basis_of) for small_table tables
    (colours near 0.5, never clamped);
  * a clamped hit is a first hit with W == float32(0.99) (there w = alpha exactly); every multi-hit scene has
    opacities <= 0.9, so o e < 0.99 always.
The frame is linear in G, so the reference is kept as D[g, p, ch] with ref[g] = sum_{p,ch} D G, and its magnitudes M.

The bound per table entry: the kernel's float32 chains (T, C, the subtraction, one reciprocal, the products) each make at
most N + O(1) roundings, and the reference's T_i differs from the kernel's by at most (i + 1) 2^-24 absolute:
    bound[g] = (2 N_max + 32) 2^-23 sum over the entry's terms of
               (e_i / ns) / (1 - alpha_i) (sum_ch |G_ch| (col_{i,ch} + C_ch) + |G_3|)
N_max the largest hit count of a ray in the frame. The wave's reduction (six adds) and the atomics' order add roundings
relative to the terms themselves, which are smaller than these magnitudes; each test prints its worst error / bound.

The check that is independent of the forward kernel is tests/test_grad_f64_gpu.py (the float64 backward of
tests/cor_f64.py, on a scene where both clamps fire behind other hits); the references here cover what that one
cannot: float32 rounding bounds per entry, GSRT_FLAG_LUT frames and the API.

Every frame here is at most 64x48 pixels.
"""
import ctypes

import numpy as np
import pytest

import gsrt
import test_features_gpu as TF
import test_sh_grad_gpu as TS
from test_feature_grad_gpu import impulse_pixels
from test_features_gpu import PLANES, Y0, _cloud, _d2h, feature_rows, noise, plane, u32, ubo_of
from test_sh_grad_gpu import MOVED, basis_of, sample_weights, small_table

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
SCENES = dict(PLANES)
SCENES["one_clamped"] = dict(k=1, opacity=1.0, scale=6.0)
# 22 Gaussians at opacity 0.9: the oracle's counts show rays stopping at 16x16 and 18x18 (213 and 265 of them at 1 spp),
# asserted in test_impulses from the weights: a stopped ray ends with T_end < 1e-3 short of the scene's last Gaussian
SCENES["stops9"] = dict(k=22, opacity=0.9, scale=1.6, spread=1.3)
_REF = {}


def view_depth(ubo, centre):
    """the kernel's float32 view depth of each centre (mul4v's third row, negated; no fma: -ffp-contract=off)"""
    m = np.asarray(ubo["model_view"][0], np.float32).reshape(-1)
    c = np.asarray(centre, np.float32)
    return -(((m[2] * c[:, 0] + m[6] * c[:, 1]) + m[10] * c[:, 2]) + m[14])


def key_order(ubo, centre):
    z = view_depth(ubo, centre)
    return np.lexsort((np.arange(len(z)), z))


def const_colour(k, seed=3):
    """a table with coefficient 0 only and its colours fl(fl(s0 Y0) + 0.5), in (0.2, 0.9)"""
    f3 = np.random.default_rng(seed).uniform(0.2, 0.9, (k, 3)).astype(np.float32)
    sh = feature_rows(f3)
    col = ((sh[:, 0, :] * Y0).astype(np.float32) + np.float32(0.5)).astype(np.float64)
    assert (col > 0).all()
    return sh, col


def linear_reference(W, order, opacity, col=None):
    """D[g, p, ch], M[g, p, ch] (float64, already divided by ns), U[g, p] (g has an unclamped hit at p), N_max.
    col: None (1), (k, 3), or a function s -> (k, 3, P)"""
    ns, k = W.shape[:2]
    P = W[0, 0].size
    D, M = np.zeros((k, P, 4)), np.zeros((k, P, 4))
    U = np.zeros((k, P), bool)
    n_max = 0
    o = np.asarray(opacity, np.float64)[order][:, None]
    for s in range(ns):
        w32 = W[s].reshape(k, P)[order]
        w = w32.astype(np.float64)
        hit = w > 0
        csum = np.cumsum(w, axis=0)
        T = 1.0 - (csum - w)
        alpha = np.where(hit, w / T, 0.0)
        t_end = 1.0 - csum[-1]
        r = 1.0 / (1.0 - alpha)
        e = alpha / o
        clamped = hit & (w32 == np.float32(0.99)) & (T == 1.0)
        use = hit & ~clamped
        er = np.where(use, e * r, 0.0) / ns
        c_all = np.ones((k, 3, 1)) if col is None else (col(s) if callable(col) else np.asarray(col, np.float64)[:, :, None])
        c_all = c_all[order]
        for ch in range(3):
            c = np.broadcast_to(c_all[:, ch], (k, P))
            after = np.cumsum(c * w, axis=0)
            C = after[-1]
            D[order, :, ch] += np.where(use, e * (T * c - (C - after) * r), 0.0) / ns
            M[order, :, ch] += er * (c + C)
        D[order, :, 3] += er * t_end
        M[order, :, 3] += er
        U[order] |= use
        n_max = max(n_max, int(hit.sum(axis=0).max()))
    return D, M, U, n_max


def evaluate(lin, G):
    D, M, _, n_max = lin
    G64 = G.astype(np.float64).reshape(-1, 4)
    return np.einsum("gpc,pc->g", D, G64), (2 * n_max + 32) * EPS * np.einsum("gpc,pc->g", M, np.abs(G64))


def ratio(err, bound):
    return float((err / np.maximum(bound, 1e-300))[bound > 0].max()) if (bound > 0).any() else 0.0


def plane_w(ctx, name, size, spp, lut=False):
    """W[s, g, y, x] of a plane scene (the weights do not depend on the colours), computed once"""
    if name in PLANES:
        return TS.plane_weights(ctx, name, size, spp, lut)  # shared with the SH gradient tests
    key = ("w", name, size, spp, lut)
    if key not in _REF:
        sc = gsrt.Scene.from_model(ctx, *plane(**SCENES[name]))
        try:
            sc.build_bvh()
            _REF[key] = sample_weights(sc, ubo_of(size, size, spp), gsrt.MODE_COR | (gsrt.FLAG_LUT if lut else 0))
        finally:
            sc.close()
    return _REF[key]


def plane_lin(ctx, name, size, spp, lut=False, colour=None):
    """the linear reference of a plane scene; colour: None or "const\""""
    key = ("lin", name, size, spp, lut, colour)
    if key not in _REF:
        model = plane(**SCENES[name])
        col = const_colour(len(model[3]))[1] if colour == "const" else None
        _REF[key] = linear_reference(plane_w(ctx, name, size, spp, lut), key_order(ubo_of(size, size, spp), model[0]),
                                     model[3], col)
    return _REF[key]


def sh_colours(B, sh):
    """s -> col[g, ch, p] = 0.5 + Y0 s_0 + sum_{q >= 1} B[s, q, p] sh[g, q, ch]"""
    sh64 = sh.astype(np.float64)

    def col(s):
        Bs = B[s].reshape(16, -1)
        c = 0.5 + float(Y0) * sh64[:, 0, :, None] + np.einsum("gqc,qp->gcp", sh64[:, 1:, :], Bs[1:])
        assert (c > 0.2).all()
        return c
    return col


def capped_cloud():
    model, _, shape = _cloud("sh3_1k")
    return model[:3] + (np.minimum(model[3], np.float32(0.9)),), shape


def cloud_lin(ctx, cam):
    """the sh3_1k cloud, opacities capped at 0.9, a small_table SH table: its scene-independent reference pieces"""
    key = ("cloud", cam)
    if key not in _REF:
        model, (w, h, spp) = capped_cloud()
        sh = small_table(len(model[3]), 71)
        ubo = ubo_of(w, h, spp, TF.MV if cam == "origin" else MOVED)
        sc = gsrt.Scene.from_model(ctx, *model, sh)
        try:
            sc.build_bvh()
            W = sample_weights(sc, ubo)
        finally:
            sc.close()
        B = basis_of(ctx, ubo)
        _REF[key] = (model, sh, ubo, W, B, linear_reference(W, key_order(ubo, model[0]), model[3], sh_colours(B, sh)))
    return _REF[key]


# ------------------------------------------------------------------------------------------------ 1: impulses, 1 spp
@pytest.mark.parametrize("size", [16, 18])
@pytest.mark.parametrize("name", ["one", "one_clamped", "stops9"])
def test_impulses(ctx, name, size):
    """One non-zero of G at a time, every channel in turn: every entry is a single term."""
    model = plane(**SCENES[name])
    k = len(model[3])
    ubo = ubo_of(size, size, 1)
    px = impulse_pixels(size)
    vals = (np.float32(0.3) + np.float32(0.17) * np.arange(16, dtype=np.float32)).astype(np.float32)
    worst = 0.0
    for lut in (False, True):
        mode = gsrt.MODE_COR | (gsrt.FLAG_LUT if lut else 0)
        for colour in (None, "const"):
            lin = plane_lin(ctx, name, size, 1, lut, colour)
            D, M, U, n_max = lin
            W = plane_w(ctx, name, size, 1, lut)[0].reshape(k, -1)
            at = [y * size + x for x, y in px]
            if name == "one_clamped":  # the impulse pixels include clamped and unclamped ones
                cl = np.array([W[0, p] == np.float32(0.99) for p in at])
                assert cl.any() and (~cl).any() and (W[0, at] > 0).all()
                assert not U[0, np.array(at)[cl]].any() and U[0, np.array(at)[~cl]].all()
            if name == "stops9" and colour is None:  # the oracle's counts: some rays stop, and the kernel blends as many hits
                st = TF.oracle_frame(model, None, size, size, 1, lut)[1]
                assert (st[..., 3] > 0).sum() > 100 and (st[..., 3] == 0).any()
                assert np.array_equal(st[..., 1].reshape(-1), (W > 0).sum(axis=0))
            sc = gsrt.Scene.from_model(ctx, *model, const_colour(k)[0] if colour else None)
            try:
                sc.build_bvh()
                plain = sc.render(ubo, mode)[0]
                for i, p in enumerate(at):
                    for ch in range(4):
                        G = np.zeros((size, size, 4), np.float32)
                        G.reshape(-1, 4)[p, ch] = vals[i]
                        got = sc.opacity_grad(ubo, G, mode)
                        assert got.shape == (k,)
                        ref, bound = evaluate(lin, G)
                        err = np.abs(got.astype(np.float64) - ref)
                        worst = max(worst, ratio(err, bound))
                        assert (err <= bound).all(), (name, size, lut, colour, i, ch)
                        assert not u32(got)[~U[:, p]].any()  # not blended, or clamped: +0 bits
                        if name == "one" and colour is None and ch == 3 and W[0, p] > 0:
                            # T_end / (1 - alpha) = 1: the result is Gs[3] e
                            e = float(W[0, p]) / float(model[3][0])
                            assert abs(float(got[0]) - float(vals[i]) * e) <= 4 * EPS * float(vals[i]) * e
                    assert _d2h(ctx.framebuffer_ptr, (size, size, 4)).tobytes() == plain.tobytes()
                assert U[:, at].any()
            finally:
                sc.close()
    print(f"opacity-grad impulses {name} {size}: worst error / bound = {worst:.4f}")


# ------------------------------------------------------------------------------------------------ 2: dense G
@pytest.mark.parametrize("spp", [1, 4, 3])
@pytest.mark.parametrize("name", ["stops9", "rounds", "past_group_list"])
def test_dense_gradient(ctx, name, spp):
    size = 18
    ubo = ubo_of(size, size, spp)
    assert (gsrt.tile_plan(ubo)["spp_lanes"] != spp) == (spp == 3)  # 3 spp run as passes
    model = plane(**SCENES[name])
    k = len(model[3])
    G = noise(size * size, 4, 300 + spp).reshape(size, size, 4)
    for colour in (None, "const"):
        ref, bound = evaluate(plane_lin(ctx, name, size, spp, False, colour), G)
        sc = gsrt.Scene.from_model(ctx, *model, const_colour(k)[0] if colour else None)
        try:
            sc.build_bvh()
            plain = sc.render(ubo, gsrt.MODE_COR)[0]
            got = sc.opacity_grad(ubo, G)
            assert _d2h(ctx.framebuffer_ptr, (size, size, 4)).tobytes() == plain.tobytes()
        finally:
            sc.close()
        err = np.abs(got.astype(np.float64) - ref)
        print(f"opacity-grad {name} spp {spp} colour {colour}: worst error / bound = {ratio(err, bound):.4f}")
        assert (err <= bound).all()
        assert np.abs(ref).max() > 0


# ------------------------------------------------------------------------------------------------ 3: cloud
@pytest.mark.parametrize("cam", ["origin", "moved"])
def test_cloud(ctx, cam):
    model, sh, ubo, W, B, lin = cloud_lin(ctx, cam)
    h, w = int(ubo["height"][0]), int(ubo["width"][0])
    G = noise(w * h, 4, 81).reshape(h, w, 4)
    ref, bound = evaluate(lin, G)
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        plain = sc.render(ubo, gsrt.MODE_COR)[0]
        got = sc.opacity_grad(ubo, G)
        assert _d2h(ctx.framebuffer_ptr, (h, w, 4)).tobytes() == plain.tobytes()
    finally:
        sc.close()
    err = np.abs(got.astype(np.float64) - ref)
    print(f"opacity-grad sh3_1k {cam}: worst error / bound = {ratio(err, bound):.4f} (N_max {lin[3]})")
    assert (err <= bound).all()
    assert np.abs(ref).max() > 0 and lin[3] > 4


# ------------------------------------------------------------------------------------------------ 4: affine identity
@pytest.mark.parametrize("spp", [1, 4])
def test_affine_identity(ctx, spp):
    """The frame is affine in one Gaussian's opacity while no cut, clamp or stop can flip:
    <G, rgba(o + d e_g) - rgba(o)> = grad[g] d, against the forward kernel alone."""
    size = 18
    ubo = ubo_of(size, size, spp)
    c, r, s, o = plane(**SCENES["rounds"])
    k = len(o)
    G = noise(size * size, 4, 91).reshape(size, size, 4)
    G64 = G.astype(np.float64)
    d = float(np.float32(0.03)) - float(np.float32(0.02))
    sc = gsrt.Scene.from_model(ctx, c, r, s, o)
    try:
        sc.build_bvh()
        assert (TS.plane_weights(ctx, "rounds", size, spp) > 0).all()
        base = sc.render(ubo, gsrt.MODE_COR)[0].astype(np.float64)
        grad = sc.opacity_grad(ubo, G).astype(np.float64)
        p0, _ = sc.download()
        worst = 0.0
        for g in (0, 1, 77, 150, 299):
            p1 = p0.copy()
            p1[g, 3] = np.float32(0.03)
            sc.update(p1)
            assert (sample_weights(sc, ubo) > 0).all()  # every Gaussian still blends at every pixel: no cut flipped
            img = sc.render(ubo, gsrt.MODE_COR)[0].astype(np.float64)
            lhs, rhs = (G64 * (img - base)).sum(), grad[g] * d
            tol = 2 * (size * size * spp + k + 24) * EPS * ((np.abs(G64) * (np.abs(base) + 1)).sum() + abs(grad[g]) * d)
            worst = max(worst, abs(lhs - rhs) / tol)
            assert abs(lhs - rhs) <= tol, (g, lhs, rhs, tol)
            assert lhs != 0.0 and rhs != 0.0
        sc.update(p0)
    finally:
        sc.close()
    print(f"opacity-grad affine identity spp {spp}: worst error / tolerance = {worst:.3g}")


# ------------------------------------------------------------------------------------------------ 5: non-finite, sentinels
def test_non_finite_and_sentinels(ctx):
    import torch

    size = 18
    ubo = ubo_of(size, size, 1)
    G = noise(size * size, 4, 5).reshape(size, size, 4)
    y, x = size // 2, size // 2 - 3
    for name in ("stops9", "one_clamped"):
        model = plane(**SCENES[name])
        k = len(model[3])
        lin = plane_lin(ctx, name, size, 1)
        U = lin[2]
        ref, bound = evaluate(lin, G)
        sc = gsrt.Scene.from_model(ctx, *model)
        try:
            sc.build_bvh()
            base = sc.opacity_grad(ubo, G).astype(np.float64)
            pixels = [(y, x)]
            if name == "one_clamped":  # one clamped and one unclamped pixel
                flat = U[0].reshape(size, size)
                pixels = [tuple(np.argwhere(~flat)[0]), tuple(np.argwhere(flat)[0])]
                assert (~flat).any() and flat.any()
            else:
                assert U[:, y * size + x].any() and not U[:, y * size + x].all()
            for py, px_ in pixels:
                for ch in (1, 3):
                    Ginf = G.copy()
                    Ginf[py, px_, ch] = np.inf
                    got = sc.opacity_grad(ubo, Ginf).astype(np.float64)
                    reach = U[:, py * size + px_]
                    assert not np.isfinite(got[reach]).any() and np.isfinite(got[~reach]).all(), (name, py, px_, ch)
                    assert (np.abs(got - base)[~reach] <= 2 * bound[~reach]).all()
            assert not u32(sc.opacity_grad(ubo, np.zeros((size, size, 3), np.float32))).any()  # all +0
            d_g = torch.from_numpy(G).to("cuda:0")
            d_t = torch.full((k + 64,), -7.5, dtype=torch.float32, device="cuda:0")
            sc.opacity_grad_async(ubo, d_g.data_ptr(), d_t.data_ptr())
            ctx.synchronize()
            t = d_t.cpu().numpy()
            assert (t[k:] == -7.5).all()
            assert (np.abs(t[:k].astype(np.float64) - ref) <= bound).all()  # the sentinels inside are overwritten
        finally:
            sc.close()


# ------------------------------------------------------------------------------------------------ 6: accumulate
def test_accumulate_adds_frames(ctx):
    import torch

    parts_lin = [cloud_lin(ctx, cam) for cam in ("origin", "moved")]
    model, sh = parts_lin[0][0], parts_lin[0][1]
    n = len(model[3])
    cams = [p[2] for p in parts_lin]
    h, w = int(cams[0]["height"][0]), int(cams[0]["width"][0])
    Gs = [noise(w * h, 4, 31 + i).reshape(h, w, 4) for i in range(2)]
    refs = [evaluate(parts_lin[i][5], Gs[i]) for i in range(2)]
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        parts = [sc.opacity_grad(cams[i], Gs[i]).astype(np.float64) for i in range(2)]
        d_t = torch.full((n,), 123.0, dtype=torch.float32, device="cuda:0")
        d_g = [torch.from_numpy(g).to("cuda:0") for g in Gs]
        sc.opacity_grad_async(cams[0], d_g[0].data_ptr(), d_t.data_ptr(), accumulate=False)  # overwrites the sentinels
        sc.opacity_grad_async(cams[1], d_g[1].data_ptr(), d_t.data_ptr(), accumulate=True)
        ctx.synchronize()
        got = d_t.cpu().numpy().astype(np.float64)
        out = np.zeros(n, np.float32)  # a host table cannot accumulate
        st = gsrt.lib.gsrt_render_opacity_grad(sc.handle, gsrt._p(cams[0]), gsrt.MODE_COR, 0, gsrt._p(Gs[0]), gsrt._p(out), 1)
        assert st == gsrt.E_ARG and "OPACITY_GRAD" in gsrt.lib.gsrt_last_error(ctx.handle).decode()
    finally:
        sc.close()
    for i in range(2):
        assert (np.abs(parts[i] - refs[i][0]) <= refs[i][1]).all()
    ref = refs[0][0] + refs[1][0]
    bound = refs[0][1] + refs[1][1]
    print(f"opacity-grad accumulate: worst error / bound = {ratio(np.abs(got - ref), bound):.4f}")
    assert (np.abs(got - ref) <= bound).all()
    assert np.abs(refs[1][0]).max() > 0


# ------------------------------------------------------------------------------------------------ 7: API
def _small_cloud():
    c, r, s, o, _ = gsrt.synth_cloud(gsrt.SYNTH_COR, 600, 21, False)
    return c, r, s, np.minimum(o, np.float32(0.9))


def _lin_of(sc, ubo, col=None):
    p, _ = sc.download()
    return linear_reference(sample_weights(sc, ubo), key_order(ubo, p[:, :3]), p[:, 3], col)


def test_opacity_grad_api(ctx):
    import torch

    c, r, s, o = _small_cloud()
    n, W, H, spp = len(o), 40, 24, 4
    sh, colours = const_colour(n, 19)
    ubo = ubo_of(W, H, spp)
    G = noise(W * H, 4, 61).reshape(H, W, 4)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    plain, _ = sc.render(ubo, gsrt.MODE_COR)
    lin = _lin_of(sc, ubo, colours)
    ref, bound = evaluate(lin, G)
    grad = sc.opacity_grad(ubo, G)  # host in, host out
    assert grad.shape == (n,) and np.abs(grad).max() > 0
    assert (np.abs(grad.astype(np.float64) - ref) <= bound).all()
    assert ctx.features_ptr() == 0 and ctx.depth_ptr() == 0 and not ctx.slot_streams()
    assert _d2h(ctx.framebuffer_ptr, (H, W, 4)).tobytes() == plain.tobytes()
    ctx.timing(1)  # gsrt_timing records the frame like any other
    sc.opacity_grad(ubo, G)
    kernel_ms, frame_ms = ctx.timing_read()
    assert len(kernel_ms) == 1 and kernel_ms[0] > 0 and frame_ms[0] >= kernel_ms[0]
    G3 = G.copy()
    G3[..., 3] = 0.0
    ref3, bound3 = evaluate(lin, G3)
    three = sc.opacity_grad(ubo, G[..., :3])  # (H, W, 3): padded with a zero alpha gradient
    assert (np.abs(three.astype(np.float64) - ref3) <= bound3).all()
    assert np.abs(ref3 - ref).max() > 10 * bound.max()
    d_g = torch.from_numpy(G).to("cuda:0")
    d_t = torch.zeros((n,), dtype=torch.float32, device="cuda:0")
    out = np.zeros(n, np.float32)
    P = ctypes.c_void_p
    for g_in, t_out in ((P(d_g.data_ptr()), P(d_t.data_ptr())), (P(d_g.data_ptr()), gsrt._p(out)), (gsrt._p(G), P(d_t.data_ptr()))):
        d_t.fill_(-3.0)
        out[:] = -3.0
        gsrt._check(gsrt.lib.gsrt_render_opacity_grad(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0, g_in, t_out, 0), ctx)
        res = out if t_out.value == out.ctypes.data else d_t.cpu().numpy()
        assert (np.abs(res.astype(np.float64) - ref) <= bound).all()

    def refused(call, what, status=gsrt.E_ARG):
        with pytest.raises(gsrt.GsrtError) as e:
            call()
        assert e.value.status == status, what
        assert "OPACITY_GRAD" in str(e.value), (what, str(e.value))
        assert sc.render(ubo, gsrt.MODE_COR)[0].tobytes() == plain.tobytes(), what

    def raw(g=G, table=out):
        gsrt._check(gsrt.lib.gsrt_render_opacity_grad(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0,
                                                      gsrt._p(g) if g is not None else None,
                                                      gsrt._p(table) if table is not None else None, 0), ctx)

    refused(lambda: sc.opacity_grad(ubo, G, gsrt.MODE_REF), "REF")
    for flag in ("STATS", "OUT_DUMP8", "DEPTH", "FEATURES", "FEATURE_GRAD", "SH_GRAD"):
        refused(lambda: sc.opacity_grad(ubo, G, gsrt.MODE_COR | getattr(gsrt, "FLAG_" + flag)), flag)
    refused(lambda: sc.opacity_grad_async(ubo, d_g.data_ptr(), d_t.data_ptr(), mode=gsrt.MODE_COR | gsrt.FLAG_STATS), "async")
    refused(lambda: sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD), "gsrt_render")
    refused(lambda: sc.render_async(ubo, gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD), "gsrt_render_async")
    refused(lambda: sc.render_depth(ubo, gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD), "render_depth")
    refused(lambda: sc.feature_grad(ubo, G, gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD), "feature_grad")
    refused(lambda: sc.sh_grad(ubo, G, gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD), "sh_grad")
    refused(lambda: sc.render_sharded_emulated(ubo, 2, gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD), "emulated shares")
    refused(lambda: raw(g=None), "NULL image")
    refused(lambda: raw(table=None), "NULL table")
    # a scene with a mesh is refused; a scene without SH rows works
    scm = gsrt.Scene.from_model(ctx, c[:100], r[:100], s[:100], o[:100], sh[:100])
    v, ix = gsrt.sphere_mesh((0.0, 0.0, -3.0), 0.5)
    scm.add_mesh(v, ix)
    scm.build_bvh()
    with pytest.raises(gsrt.GsrtError) as e:
        scm.opacity_grad(ubo, G)
    assert e.value.status == gsrt.E_ARG and "OPACITY_GRAD" in str(e.value)
    scm.close()
    scn = gsrt.Scene.from_model(ctx, c, r, s, o)
    scn.build_bvh()
    refn, boundn = evaluate(_lin_of(scn, ubo), G)
    gotn = scn.opacity_grad(ubo, G).astype(np.float64)
    scn.close()
    assert (np.abs(gotn - refn) <= boundn).all() and np.abs(refn - ref).max() > 10 * max(bound.max(), boundn.max())
    assert (np.abs(sc.opacity_grad(ubo, G).astype(np.float64) - ref) <= bound).all()  # and gradients as before

    # an update + refit between two queued gradient frames changes the second only
    p, a = sc.download()
    d = np.random.default_rng(5).normal(0.0, 2e-2, (n, 3)).astype(np.float32)
    p1, a1 = p.copy(), a.copy()
    p1[:, :3] += d
    a1[:, :3] += d
    a1[:, 3:] += d
    d_a = torch.zeros((n,), dtype=torch.float32, device="cuda:0")
    d_b = torch.zeros((n,), dtype=torch.float32, device="cuda:0")
    sc.opacity_grad_async(ubo, d_g.data_ptr(), d_a.data_ptr())
    sc.update(p1, a1)
    sc.refit_bvh()
    sc.opacity_grad_async(ubo, d_g.data_ptr(), d_b.data_ptr())
    ctx.synchronize()
    ref1, bound1 = evaluate(_lin_of(sc, ubo, colours), G)  # the moved scene's own reference
    assert (np.abs(d_a.cpu().numpy().astype(np.float64) - ref) <= bound).all()
    assert (np.abs(d_b.cpu().numpy().astype(np.float64) - ref1) <= bound1).all()
    assert np.abs(ref1 - ref).max() > 10 * max(bound.max(), bound1.max())
    sc.close()


def test_opacity_grad_refused_on_sharded_frames():
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 5000, 21, True)
    with gsrt.Context(0) as cx:
        sc = gsrt.Scene.from_model(cx, c, r, s, o, sh)
        sc.build_bvh()
        ubo = ubo_of(40, 24, 4)
        plain, _ = sc.render(ubo, gsrt.MODE_COR)
        cx.comm_init_loopback()
        for call in (lambda: sc.render_sharded(ubo, gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD),
                     lambda: sc.render_sharded_async(ubo, gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD)):
            with pytest.raises(gsrt.GsrtError) as e:
                call()
            assert e.value.status == gsrt.E_ARG and "OPACITY_GRAD" in str(e.value)
            assert sc.render_sharded(ubo, gsrt.MODE_COR).tobytes() == plain.tobytes()


# ------------------------------------------------------------------------------------------------ 8: ordering
@pytest.fixture(params=["adaptive", "0", "1"])
def slot_knob(request, monkeypatch):
    if request.param != "adaptive":
        monkeypatch.setenv("GSRT_DEBUG_SLOT_STREAMS", request.param)
    return request.param


def test_frames_around_opacity_gradient_frames_match_sync(ctx, slot_knob):
    """Plain, depth, feature, feature-gradient, SH-gradient and opacity-gradient frames queued without a sync in between:
    the images match their synchronous renders byte for byte, whatever the plain frames' slot-stream choice, and the
    opacity tables are finite and within twice the bound of the synchronous result."""
    import torch

    model, sh, ubo, _, _, lin = cloud_lin(ctx, "origin")
    n, C = len(model[3]), 7
    H, W = int(ubo["height"][0]), int(ubo["width"][0])
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    sc.build_bvh()
    sc.set_features(noise(n, C, 53))
    want_p = sc.render(ubo, gsrt.MODE_COR)[0]
    want_d = sc.render_depth(ubo)
    want_f = sc.render_features(ubo)
    G = noise(W * H, 4, 3).reshape(H, W, 4)
    Gf = noise(W * H, C, 4).reshape(H, W, C)
    want_o = sc.opacity_grad(ubo, G).astype(np.float64)
    ref, bound = evaluate(lin, G)
    assert (np.abs(want_o - ref) <= bound).all()
    d_g, d_gf = torch.from_numpy(G).to("cuda:0"), torch.from_numpy(Gf).to("cuda:0")
    kinds = ["plain", "opgrad", "plain", "depth", "opgrad", "feat", "grad", "opgrad", "shgrad", "plain", "plain", "opgrad",
             "feat", "depth"]
    shape = {"opgrad": (n,), "shgrad": (n, 16, 3), "grad": (n, C), "feat": (H, W, C), "depth": (H, W, 1), "plain": (1,)}
    out = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in kinds]
    aux = [torch.zeros(shape[kd], dtype=torch.float32, device="cuda:0") for kd in kinds]
    for i, kd in enumerate(kinds):
        if kd == "plain":
            sc.render_async(ubo, gsrt.MODE_COR, d_rgba=out[i].data_ptr())
        elif kd == "depth":
            sc.render_depth_async(ubo, d_rgba=out[i].data_ptr(), d_depth=aux[i].data_ptr())
        elif kd == "feat":
            sc.render_features_async(ubo, d_rgba=out[i].data_ptr(), d_feat=aux[i].data_ptr())
        elif kd == "grad":
            sc.feature_grad_async(ubo, d_gf.data_ptr(), C, aux[i].data_ptr())
        elif kd == "shgrad":
            sc.sh_grad_async(ubo, d_g.data_ptr(), aux[i].data_ptr())
        else:
            sc.opacity_grad_async(ubo, d_g.data_ptr(), aux[i].data_ptr())
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
        elif kd == "opgrad":
            got = aux[i].cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all(), i
            assert (np.abs(got - want_o) <= 2 * bound).all(), i
        else:
            assert np.isfinite(aux[i].cpu().numpy()).all(), i
    assert np.abs(want_o).max() > 0
    sc.close()


# ------------------------------------------------------------------------------------------------ 9: autograd
def test_autograd_matches_the_direct_gradients(ctx):
    import torch

    from gsrt.autograd import render_rgba

    model, sh, ubo, Wg, B, lin = cloud_lin(ctx, "origin")
    n = len(model[3])
    h, w = int(ubo["height"][0]), int(ubo["width"][0])
    G = noise(w * h, 4, 97).reshape(h, w, 4)
    d_G = torch.from_numpy(G).to("cuda:0")
    # a scene created with other opacities and SH rows: the forward puts the tensors' values in
    sc = gsrt.Scene.from_model(ctx, model[0], model[1], model[2], np.full(n, 0.5, np.float32), small_table(n, 5))
    made = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        made.build_bvh()
        opacity = torch.from_numpy(model[3]).to("cuda:0").requires_grad_(True)
        table = torch.from_numpy(sh).to("cuda:0").requires_grad_(True)
        rgba = render_rgba(sc, ubo, opacity, table)
        assert rgba.detach().cpu().numpy().tobytes() == made.render(ubo, gsrt.MODE_COR)[0].tobytes()
        (rgba * d_G).sum().backward()  # the upstream gradient is G itself
        ref_o, bound_o = evaluate(lin, G)
        ref_s, bound_s = TS.reference(Wg, B, np.ones((n, 3), bool), G)
        direct_o = sc.opacity_grad(ubo, G).astype(np.float64)
        direct_s = sc.sh_grad(ubo, G).astype(np.float64)
        back_o = opacity.grad.cpu().numpy().astype(np.float64)
        back_s = table.grad.cpu().numpy().astype(np.float64)
        assert back_o.shape == (n,) and back_s.shape == (n, 16, 3)
        print(f"opacity-grad autograd: worst error / bound = {ratio(np.abs(back_o - ref_o), bound_o):.4f}")
        assert (np.abs(back_o - ref_o) <= bound_o).all() and (np.abs(direct_o - ref_o) <= bound_o).all()
        assert (np.abs(back_o - direct_o) <= 2 * bound_o).all()
        assert (np.abs(back_s - ref_s) <= bound_s).all() and (np.abs(direct_s - ref_s) <= bound_s).all()
        assert (np.abs(back_s - direct_s) <= 2 * bound_s).all()
        assert np.abs(ref_o).max() > 0 and np.abs(ref_s).max() > 0
        # sh=None: only the opacity gradient, of the scene's rows as they are
        opacity.grad = None
        rgba = render_rgba(sc, ubo, opacity)
        assert rgba.detach().cpu().numpy().tobytes() == made.render(ubo, gsrt.MODE_COR)[0].tobytes()
        (rgba * d_G).sum().backward()
        assert (np.abs(opacity.grad.cpu().numpy().astype(np.float64) - ref_o) <= bound_o).all()
        # a second forward with changed opacities: the frame of a scene created with them
        other = np.random.default_rng(3).uniform(0.05, 0.9, n).astype(np.float32)
        with torch.no_grad():
            rgba = render_rgba(sc, ubo, torch.from_numpy(other).to("cuda:0"), table)
        fresh = gsrt.Scene.from_model(ctx, model[0], model[1], model[2], other, sh)
        try:
            fresh.build_bvh()
            assert rgba.cpu().numpy().tobytes() == fresh.render(ubo, gsrt.MODE_COR)[0].tobytes()
            assert rgba.cpu().numpy().tobytes() != made.render(ubo, gsrt.MODE_COR)[0].tobytes()
        finally:
            fresh.close()
    finally:
        sc.close()
        made.close()
