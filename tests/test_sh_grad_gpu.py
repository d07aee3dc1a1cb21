"""SH gradient frames (GSRT_FLAG_SH_GRAD, gsrt_render_sh_grad) and gsrt_scene_set_sh: the backward of a COR colour frame
to the SH table, grad[g, q, ch] = sum over the hits i of Gaussian g with an unclamped channel of w_i Y_q G[p, ch] / ns.

The reference of every numeric check is built from forward kernels that existing tests tie to the oracle:
  * W_{g,s}[p], Gaussian g's weight in sample s of pixel p, from one-hot feature frames at 1 spp (weights_of); sample s of
    an ns-spp frame is a 1-spp frame whose random_seed is the pixel LCG advanced by 2 s draws (test_samples_are_frames);
  * B_{q,s}[p], the kernel's own SH basis at the pixel, from plain frames of a one-Gaussian scene that covers every pixel
    with coefficient q of all three channels set to 0.25: B = (rgb - 0.5 W) / (0.25 W), within 4 2^-23 of the kernel's;
  * the clamp mask M[g, ch] from the table alone: |s_q| <= 0.02 for q >= 1 bounds the ray-dependent part by 0.225, so
    s_0 = +1 never clamps (a >= 0.78 - 0.225) and s_0 = -4 always does (a <= 0.5 - 1.128 + 0.225).
ref[g, q, ch] = sum_{p,s} W B M G / ns in float64, bound (N_g + 8) 2^-23 sum W |B| |G| / ns + 4 2^-23 sum W |G| / ns.

The check that is independent of the forward kernel is tests/test_grad_f64_gpu.py (the float64 backward of
tests/cor_f64.py, on a scene where both clamps fire behind other hits); the references here cover what that one
cannot: float32 rounding bounds per entry, GSRT_FLAG_LUT frames and the API.

Every frame here is at most 64x48 pixels.
"""
import ctypes

import numpy as np
import pytest

import cor_f64 as F
import gsrt
import test_features_gpu as TF
from test_feature_grad_gpu import impulse_pixels, weights_of
from test_features_gpu import PLANES, _cloud, _d2h, noise, plane, u32, ubo_of

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
MOVED = gsrt.lookat((0.05, -0.03, 0.1), (0.02, 0, -1))
_REF = {}


def sample_ubo(ubo, s):
    """the 1-spp camera of sample s of ubo's frame: the pixel LCG advanced by 2 s draws (cor_f64.jitter's recurrence)"""
    u = ubo.copy()
    seed = int(ubo["random_seed"][0])
    for _ in range(2 * s):
        seed = (1664525 * seed + 1013904223) & 0xFFFFFFFF
    u["samples"][0] = 1
    u["total_samples"][0] = 1
    u["random_seed"][0] = seed
    return u


def delta_table(n, q, v=0.25):
    sh = np.zeros((n, 16, 3), np.float32)
    sh[:, q, :] = v
    return sh


def basis_of(ctx, ubo):
    """B[s, q, y, x] (float64): the kernel's SH basis of sample s at each pixel, from the one-Gaussian covering scene"""
    ns, h, w = int(ubo["samples"][0]), int(ubo["height"][0]), int(ubo["width"][0])
    key = ("basis", w, h, ns, int(ubo["random_seed"][0]), ubo["model_view"].tobytes())
    if key not in _REF:
        B = np.zeros((ns, 16, h, w))
        sc = gsrt.Scene.from_model(ctx, *plane(k=1, opacity=0.8, scale=6.0))
        try:
            sc.build_bvh()
            for s in range(ns):
                us = sample_ubo(ubo, s)
                W1 = weights_of(sc, us)[0][0].astype(np.float64)
                assert (W1 > 0).all()
                for q in range(16):
                    sc.set_sh(delta_table(1, q))
                    rgb = sc.render(us, gsrt.MODE_COR)[0][..., :3].astype(np.float64)
                    assert (rgb == rgb[..., :1]).all()
                    B[s, q] = (rgb[..., 0] - 0.5 * W1) / (0.25 * W1)
                sc.set_sh(None)
        finally:
            sc.close()
        _REF[key] = B
    return _REF[key]


def sample_weights(sc, ubo, mode=gsrt.MODE_COR):
    """W[s, g, y, x] (float32) of the scene's frame, per sample; replaces the scene's feature table"""
    ns = int(ubo["samples"][0])
    W = np.stack([weights_of(sc, sample_ubo(ubo, s), mode)[0] for s in range(ns)])
    sc.set_features(None)
    return W


def plane_weights(ctx, name, size, spp, lut=False):
    key = ("w", name, size, spp, lut)
    if key not in _REF:
        sc = gsrt.Scene.from_model(ctx, *plane(**PLANES[name]))
        try:
            sc.build_bvh()
            _REF[key] = sample_weights(sc, ubo_of(size, size, spp), gsrt.MODE_COR | (gsrt.FLAG_LUT if lut else 0))
        finally:
            sc.close()
    return _REF[key]


def reference(W, B, M, G):
    """ref[g, q, ch] and its bound from W[s, g, y, x], B[s, q, y, x], M[g, ch] (bool) and G[y, x, >= 3]"""
    ns, k = W.shape[:2]
    W64 = W.astype(np.float64).reshape(ns, k, -1)
    G64 = G[..., :3].astype(np.float64).reshape(-1, 3) / ns
    ref = np.zeros((k, 16, 3))
    wbg = np.zeros((k, 16, 3))
    wg = np.zeros((k, 3))
    for s in range(ns):
        Bs = B[s].reshape(16, -1)
        BG = (Bs.T[:, :, None] * G64[:, None, :]).reshape(-1, 48)  # [p, (q, ch)]
        ref += (W64[s] @ BG).reshape(k, 16, 3)
        wbg += (W64[s] @ np.abs(BG)).reshape(k, 16, 3)
        wg += W64[s] @ np.abs(G64)
    m = M.astype(np.float64)[:, None, :]
    ng = ns * (W > 0).any(axis=0).sum(axis=(1, 2))
    bound = ((ng[:, None, None] + 8) * EPS * wbg + 4 * EPS * wg[:, None, :]) * m
    return ref * m, bound


def masked_table(k, seed, all_pass=False):
    """an SH table with small random higher coefficients and s_0 in {+1, -4} per (g, ch), and its clamp mask"""
    rng = np.random.default_rng(seed)
    sh = rng.uniform(-0.02, 0.02, (k, 16, 3)).astype(np.float32)
    M = np.ones((k, 3), bool) if all_pass else rng.random((k, 3)) < 0.6
    sh[:, 0, :] = np.where(M, np.float32(1.0), np.float32(-4.0))
    return sh, M


def small_table(n, seed):
    return np.random.default_rng(seed).uniform(-0.02, 0.02, (n, 16, 3)).astype(np.float32)


def test_basis_stays_below_one():
    """|Y_q| <= 0.7464 on the unit sphere (Y_12 at z = +-1), so col = fma(Y, 0.25, 0.5) lies in (0.22, 0.78)"""
    d = np.random.default_rng(1).normal(size=(200000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = np.concatenate([d, np.eye(3), -np.eye(3)])
    m = np.abs(F.sh_basis(d)).max()
    assert 0.74 < m <= 0.7464, m


# ------------------------------------------------------------------------------------------------ 0: samples are frames
@pytest.mark.parametrize("spp", [4, 3])
@pytest.mark.parametrize("name", ["stops", "rounds", "past_group_list"])
def test_samples_are_frames(ctx, name, spp):
    """The mean over s of the ns 1-spp plain frames at the advanced seeds is the ns-spp frame, within (ns + 2) 2^-23
    relative per channel"""
    model = plane(**PLANES[name])
    ubo = ubo_of(18, 18, spp)
    assert (gsrt.tile_plan(ubo)["spp_lanes"] != spp) == (spp == 3)
    sc = gsrt.Scene.from_model(ctx, *model, masked_table(len(model[3]), 5)[0])
    try:
        sc.build_bvh()
        whole = sc.render(ubo, gsrt.MODE_COR)[0].astype(np.float64)
        parts = np.stack([sc.render(sample_ubo(ubo, s), gsrt.MODE_COR)[0].astype(np.float64) for s in range(spp)])
    finally:
        sc.close()
    mean = parts.mean(axis=0)
    assert mean.max() > 0 and np.abs(parts[0] - parts[1]).max() > 0
    assert (np.abs(mean - whole) <= (spp + 2) * EPS * np.abs(mean)).all()


# ------------------------------------------------------------------------------------------------ 1: set_sh
def test_set_sh_matches_creation(ctx):
    import torch

    model, sh, (w, h, spp) = _cloud("sh3_1k")
    ubo = ubo_of(w, h, spp)
    other = masked_table(len(model[3]), 9)[0]
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    made = gsrt.Scene.from_model(ctx, *model, other)
    bare = gsrt.Scene.from_model(ctx, *model)
    try:
        for s in (sc, made, bare):
            s.build_bvh()
        want_sh, want_other, want_bare = (s.render(ubo, gsrt.MODE_COR)[0] for s in (sc, made, bare))
        assert want_sh.tobytes() != want_other.tobytes() != want_bare.tobytes()
        # frames queued before the call are unchanged
        d_out = torch.zeros((2, h, w, 4), dtype=torch.float32, device="cuda:0")
        sc.render_async(ubo, gsrt.MODE_COR, d_rgba=d_out[0].data_ptr())
        sc.render_async(ubo, gsrt.MODE_COR, d_rgba=d_out[1].data_ptr())
        sc.set_sh(other)  # a host array
        assert d_out[0].cpu().numpy().tobytes() == want_sh.tobytes() == d_out[1].cpu().numpy().tobytes()
        assert sc.render(ubo, gsrt.MODE_COR)[0].tobytes() == want_other.tobytes()
        sc.set_sh(None)
        assert sc.render(ubo, gsrt.MODE_COR)[0].tobytes() == want_bare.tobytes()
        d_sh = torch.from_numpy(np.ascontiguousarray(sh, np.float32)).to("cuda:0")
        torch.cuda.synchronize()
        sc.set_sh(d_sh.data_ptr())  # a device tensor, into a scene without rows
        assert sc.render(ubo, gsrt.MODE_COR)[0].tobytes() == want_sh.tobytes()
        sc.set_sh(other.reshape(-1, 48))
        assert sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_LUT)[0].tobytes() == made.render(ubo, gsrt.MODE_COR | gsrt.FLAG_LUT)[0].tobytes()
        d_other = torch.from_numpy(other).to("cuda:0")
        torch.cuda.synchronize()
        bare.set_sh(d_other.data_ptr())
        assert bare.render(ubo, gsrt.MODE_COR)[0].tobytes() == want_other.tobytes()
    finally:
        for s in (sc, made, bare):
            s.close()


# ------------------------------------------------------------------------------------------------ 2: impulses, 1 spp
@pytest.mark.parametrize("size", [16, 18])
@pytest.mark.parametrize("name", ["one", "stops"])
def test_impulses_one_sample(ctx, name, size):
    """One non-zero of G per colour channel: every entry is a single term, so |got - ref| <= (2 + 4) 2^-23 W |G| (the two
    products and the basis term); Gaussians the pixel does not blend hold +0; the framebuffer is the plain frame's."""
    model = plane(**PLANES[name])
    k = len(model[3])
    ubo = ubo_of(size, size, 1)
    sh, M = masked_table(k, 11, all_pass=True)
    B = basis_of(ctx, ubo)[0]
    px = impulse_pixels(size)
    vals = (np.float32(0.3) + np.float32(0.17) * np.arange(16, dtype=np.float32)).astype(np.float32)
    for lut in (False, True):
        mode = gsrt.MODE_COR | (gsrt.FLAG_LUT if lut else 0)
        W = plane_weights(ctx, name, size, 1, lut)[0]
        sc = gsrt.Scene.from_model(ctx, *model, sh)
        try:
            sc.build_bvh()
            plain = sc.render(ubo, mode)[0]
            seen = False
            for i0 in range(0, 16, 3):
                G = np.zeros((size, size, 4), np.float32)
                G[..., 3] = 5.0  # alpha's gradient is ignored
                for ch, i in enumerate(range(i0, min(i0 + 3, 16))):
                    G[px[i][1], px[i][0], ch] = vals[i]
                got = sc.sh_grad(ubo, G, mode)
                assert got.shape == (k, 16, 3)
                assert _d2h(ctx.framebuffer_ptr, (size, size, 4)).tobytes() == plain.tobytes()
                for ch, i in enumerate(range(i0, min(i0 + 3, 16))):
                    x, y = px[i]
                    w = W[:, y, x].astype(np.float64)
                    ref = w[:, None] * B[None, :, y, x] * float(vals[i])
                    tol = 6 * EPS * w * float(vals[i])
                    assert (np.abs(got[:, :, ch] - ref) <= tol[:, None]).all(), (name, size, lut, i)
                    assert not u32(got[:, :, ch])[w == 0].any()
                    seen = seen or (w > 0).any()
                for ch in range(min(i0 + 3, 16) - i0, 3):
                    assert not u32(got[:, :, ch]).any()
            assert seen
        finally:
            sc.close()


# ------------------------------------------------------------------------------------------------ 3: dense G
@pytest.mark.parametrize("spp", [1, 4, 3])
@pytest.mark.parametrize("name", ["stops", "rounds", "past_group_list"])
def test_dense_gradient(ctx, name, spp):
    size = 18
    ubo = ubo_of(size, size, spp)
    model = plane(**PLANES[name])
    k = len(model[3])
    sh, M = masked_table(k, 13)
    G = noise(size * size, 4, 200 + spp).reshape(size, size, 4)
    W = plane_weights(ctx, name, size, spp)
    ref, bound = reference(W, basis_of(ctx, ubo), M, G)
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        got = sc.sh_grad(ubo, G)
    finally:
        sc.close()
    hit = (W > 0).any(axis=(0, 2, 3))
    assert M[hit].any() and (~M[hit]).any()
    err = np.abs(got.astype(np.float64) - ref)
    print(f"sh-grad {name} spp {spp}: worst error / bound = {(err / np.maximum(bound, 1e-300))[bound > 0].max():.4f}")
    assert (err <= bound).all()
    assert not u32(got)[np.broadcast_to(~M[:, None, :], got.shape)].any()  # a clamped channel: +0
    assert np.abs(ref).max() > 0


# ------------------------------------------------------------------------------------------------ 4: clouds
@pytest.mark.parametrize("cam", ["origin", "moved"])
@pytest.mark.parametrize("name", ["10k", "20k"])
def test_clouds_affine_identity(ctx, name, cam):
    """Without a clamp the frame is affine in the table: <G, rgb(sh0 + d) - rgb(sh0)> = <grad(sh0), d>, within
    2 (W H ns + n_max + 24) 2^-23 (sum_p |G[p]| alpha[p] + sum |grad| |d|)"""
    model, _, (w, h, spp) = _cloud(name)
    n = len(model[3])
    mv = TF.MV if cam == "origin" else MOVED
    ubo = ubo_of(w, h, spp, mv)
    _, st = TF.oracle_frame(model, None, w, h, spp, False, mv)
    n_max = int(st[..., 1].max())
    sh0 = small_table(n, 41)
    deltas = [small_table(n, 43 + j) for j in range(4)]
    ind = np.zeros((n, 16, 3), np.float32)
    ind[np.random.default_rng(47).random(n) < 0.5, 6, :] = 0.02
    deltas.append(ind)
    G = noise(w * h, 4, 49).reshape(h, w, 4)
    G64 = G[..., :3].astype(np.float64)
    sc = gsrt.Scene.from_model(ctx, *model, sh0)
    try:
        sc.build_bvh()
        base = sc.render(ubo, gsrt.MODE_COR)[0].astype(np.float64)
        grad = sc.sh_grad(ubo, G).astype(np.float64)
        assert _d2h(ctx.framebuffer_ptr, (h, w, 4)).astype(np.float64).tobytes() == base.tobytes()
        moved = []
        for d in deltas:
            sh1 = (sh0 + d).astype(np.float32)
            sc.set_sh(sh1)
            moved.append((sh1.astype(np.float64) - sh0.astype(np.float64), sc.render(ubo, gsrt.MODE_COR)[0].astype(np.float64)))
    finally:
        sc.close()
    k = 2 * (w * h * spp + n_max + 24) * EPS
    worst = 0.0
    for d64, img in moved:
        lhs = (G64 * (img[..., :3] - base[..., :3])).sum()
        rhs = (grad * d64).sum()
        bound = k * ((np.abs(G64) * base[..., 3:]).sum() + (np.abs(grad) * np.abs(d64)).sum())
        worst = max(worst, abs(lhs - rhs) / bound)
        assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
        assert lhs != 0.0 and rhs != 0.0
    print(f"sh-grad {name} {cam}: affine identity worst error / bound = {worst:.4f}")


# ------------------------------------------------------------------------------------------------ 5: non-finite, sentinels
def test_masks_and_non_finite(ctx):
    import torch

    size = 18
    ubo = ubo_of(size, size, 1)
    model = plane(**PLANES["stops"])
    k = len(model[3])
    sh, M = masked_table(k, 13)
    W = plane_weights(ctx, "stops", size, 1)
    G = noise(size * size, 4, 5).reshape(size, size, 4)
    y, x = size // 2, size // 2 - 3
    hit = W[0, :, y, x] > 0
    assert (hit & M[:, 1]).any() and (hit & ~M[:, 1]).any() and not hit.all()
    Ginf = G.copy()
    Ginf[y, x, 1] = np.inf
    ref, bound = reference(W, basis_of(ctx, ubo), M, G)
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        base = sc.sh_grad(ubo, G).astype(np.float64)
        got = sc.sh_grad(ubo, Ginf).astype(np.float64)
        reach = np.zeros((k, 16, 3), bool)
        reach[hit & M[:, 1], :, 1] = True
        assert not np.isfinite(got[reach]).any() and np.isfinite(got[~reach]).all()
        assert (np.abs(got - base)[~reach] <= 2 * bound[~reach]).all()
        assert not u32(sc.sh_grad(ubo, np.zeros((size, size, 3), np.float32))).any()  # all +0
        d_g = torch.from_numpy(G).to("cuda:0")
        d_t = torch.full((k * 48 + 64,), -7.5, dtype=torch.float32, device="cuda:0")
        sc.sh_grad_async(ubo, d_g.data_ptr(), d_t.data_ptr())
        ctx.synchronize()
        t = d_t.cpu().numpy()
        assert (t[k * 48:] == -7.5).all()
        assert (np.abs(t[:k * 48].reshape(k, 16, 3).astype(np.float64) - ref) <= bound).all()  # sentinels inside overwritten
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------ 6: accumulate
def test_accumulate_adds_frames(ctx):
    import torch

    model, _, (w, h, spp) = _cloud("sh3_1k")
    n = len(model[3])
    sh, M = masked_table(n, 17)
    cams = [ubo_of(w, h, spp), ubo_of(w, h, spp, MOVED)]
    Gs = [noise(w * h, 4, 31 + i).reshape(h, w, 4) for i in range(2)]
    sc = gsrt.Scene.from_model(ctx, *model, sh)
    try:
        sc.build_bvh()
        refs = [reference(sample_weights(sc, cams[i]), basis_of(ctx, cams[i]), M, Gs[i]) for i in range(2)]
        parts = [sc.sh_grad(cams[i], Gs[i]).astype(np.float64) for i in range(2)]
        d_t = torch.full((n, 16, 3), 123.0, dtype=torch.float32, device="cuda:0")
        d_g = [torch.from_numpy(g).to("cuda:0") for g in Gs]
        sc.sh_grad_async(cams[0], d_g[0].data_ptr(), d_t.data_ptr(), accumulate=False)  # overwrites the sentinels
        sc.sh_grad_async(cams[1], d_g[1].data_ptr(), d_t.data_ptr(), accumulate=True)
        ctx.synchronize()
        got = d_t.cpu().numpy().astype(np.float64)
        out = np.zeros((n, 16, 3), np.float32)  # a host table cannot accumulate
        st = gsrt.lib.gsrt_render_sh_grad(sc.handle, gsrt._p(cams[0]), gsrt.MODE_COR, 0, gsrt._p(Gs[0]), gsrt._p(out), 1)
        assert st == gsrt.E_ARG and "SH_GRAD" in gsrt.lib.gsrt_last_error(ctx.handle).decode()
    finally:
        sc.close()
    for i in range(2):
        assert (np.abs(parts[i] - refs[i][0]) <= refs[i][1]).all()
    ref = refs[0][0] + refs[1][0]
    bound = refs[0][1] + refs[1][1] + EPS * np.abs(ref)
    print(f"sh-grad accumulate: worst error / bound = {(np.abs(got - ref) / np.maximum(bound, 1e-300))[bound > 0].max():.4f}")
    assert (np.abs(got - ref) <= bound).all()
    assert (np.abs(got - (parts[0] + parts[1])) <= 2 * bound).all()
    assert np.abs(refs[1][0]).max() > 0


# ------------------------------------------------------------------------------------------------ 7: API and ordering
def test_sh_grad_api(ctx):
    import torch

    c, r, s, o, _ = gsrt.synth_cloud(gsrt.SYNTH_COR, 2000, 21, False)
    n, W, H, spp = len(o), 40, 24, 4
    sh, M = masked_table(n, 19)
    ubo = ubo_of(W, H, spp)
    G = noise(W * H, 4, 61).reshape(H, W, 4)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    plain, _ = sc.render(ubo, gsrt.MODE_COR)
    B = basis_of(ctx, ubo)
    ref, bound = reference(sample_weights(sc, ubo), B, M, G)
    grad = sc.sh_grad(ubo, G)  # host in, host out
    assert grad.shape == (n, 16, 3) and np.abs(grad).max() > 0
    assert (np.abs(grad.astype(np.float64) - ref) <= bound).all()
    assert ctx.features_ptr() == 0 and ctx.depth_ptr() == 0 and not ctx.slot_streams()
    assert _d2h(ctx.framebuffer_ptr, (H, W, 4)).tobytes() == plain.tobytes()
    three = sc.sh_grad(ubo, G[..., :3])  # (H, W, 3): padded
    assert (np.abs(three.astype(np.float64) - ref) <= bound).all()
    d_g = torch.from_numpy(G).to("cuda:0")
    d_t = torch.zeros((n, 16, 3), dtype=torch.float32, device="cuda:0")
    out = np.zeros((n, 16, 3), np.float32)
    P = ctypes.c_void_p
    for g_in, t_out in ((P(d_g.data_ptr()), P(d_t.data_ptr())), (P(d_g.data_ptr()), gsrt._p(out)), (gsrt._p(G), P(d_t.data_ptr()))):
        d_t.fill_(-3.0)
        out[:] = -3.0
        gsrt._check(gsrt.lib.gsrt_render_sh_grad(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0, g_in, t_out, 0), ctx)
        res = out if t_out.value == out.ctypes.data else d_t.cpu().numpy()
        assert (np.abs(res.astype(np.float64) - ref) <= bound).all()

    def refused(call, what, status=gsrt.E_ARG):
        with pytest.raises(gsrt.GsrtError) as e:
            call()
        assert e.value.status == status, what
        assert "SH_GRAD" in str(e.value), (what, str(e.value))
        assert sc.render(ubo, gsrt.MODE_COR)[0].tobytes() == plain.tobytes(), what

    def raw(g=G, table=out):
        gsrt._check(gsrt.lib.gsrt_render_sh_grad(sc.handle, gsrt._p(ubo), gsrt.MODE_COR, 0, gsrt._p(g) if g is not None else None,
                                                 gsrt._p(table) if table is not None else None, 0), ctx)

    refused(lambda: sc.sh_grad(ubo, G, gsrt.MODE_REF), "REF")
    for flag in ("STATS", "OUT_DUMP8", "DEPTH", "FEATURES", "FEATURE_GRAD"):
        refused(lambda: sc.sh_grad(ubo, G, gsrt.MODE_COR | getattr(gsrt, "FLAG_" + flag)), flag)
    refused(lambda: sc.sh_grad_async(ubo, d_g.data_ptr(), d_t.data_ptr(), mode=gsrt.MODE_COR | gsrt.FLAG_STATS), "async")
    refused(lambda: sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_SH_GRAD), "gsrt_render")
    refused(lambda: sc.render_async(ubo, gsrt.MODE_COR | gsrt.FLAG_SH_GRAD), "gsrt_render_async")
    refused(lambda: sc.render_depth(ubo, gsrt.MODE_COR | gsrt.FLAG_SH_GRAD), "render_depth")
    refused(lambda: sc.feature_grad(ubo, G, gsrt.MODE_COR | gsrt.FLAG_SH_GRAD), "feature_grad")
    refused(lambda: sc.render_sharded_emulated(ubo, 2, gsrt.MODE_COR | gsrt.FLAG_SH_GRAD), "emulated shares")
    refused(lambda: raw(g=None), "NULL image")
    refused(lambda: raw(table=None), "NULL table")
    # a scene with a mesh; a scene without SH rows
    scm = gsrt.Scene.from_model(ctx, c[:100], r[:100], s[:100], o[:100], sh[:100])
    v, ix = gsrt.sphere_mesh((0.0, 0.0, -3.0), 0.5)
    scm.add_mesh(v, ix)
    scm.build_bvh()
    with pytest.raises(gsrt.GsrtError) as e:
        scm.sh_grad(ubo, G)
    assert e.value.status == gsrt.E_ARG and "SH_GRAD" in str(e.value)
    scm.close()
    scn = gsrt.Scene.from_model(ctx, c[:100], r[:100], s[:100], o[:100])
    scn.build_bvh()
    with pytest.raises(gsrt.GsrtError) as e:
        scn.sh_grad(ubo, G)
    assert e.value.status == gsrt.E_STATE and "SH_GRAD" in str(e.value)
    scn.close()
    assert (np.abs(sc.sh_grad(ubo, G).astype(np.float64) - ref) <= bound).all()  # and gradients as before

    # an update + refit between two queued gradient frames changes the second only
    p, a = sc.download()
    d = np.random.default_rng(5).normal(0.0, 2e-2, (n, 3)).astype(np.float32)
    p1, a1 = p.copy(), a.copy()
    p1[:, :3] += d
    a1[:, :3] += d
    a1[:, 3:] += d
    d_a = torch.zeros((n, 16, 3), dtype=torch.float32, device="cuda:0")
    d_b = torch.zeros((n, 16, 3), dtype=torch.float32, device="cuda:0")
    sc.sh_grad_async(ubo, d_g.data_ptr(), d_a.data_ptr())
    sc.update(p1, a1)
    sc.refit_bvh()
    sc.sh_grad_async(ubo, d_g.data_ptr(), d_b.data_ptr())
    ctx.synchronize()
    ref1, bound1 = reference(sample_weights(sc, ubo), B, M, G)  # the moved scene's own reference
    assert (np.abs(d_a.cpu().numpy().astype(np.float64) - ref) <= bound).all()
    assert (np.abs(d_b.cpu().numpy().astype(np.float64) - ref1) <= bound1).all()
    assert np.abs(ref1 - ref).max() > 10 * max(bound.max(), bound1.max())
    sc.close()


def test_sh_grad_refused_on_sharded_frames():
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 5000, 21, True)
    with gsrt.Context(0) as cx:
        sc = gsrt.Scene.from_model(cx, c, r, s, o, sh)
        sc.build_bvh()
        ubo = ubo_of(40, 24, 4)
        plain, _ = sc.render(ubo, gsrt.MODE_COR)
        cx.comm_init_loopback()
        for call in (lambda: sc.render_sharded(ubo, gsrt.MODE_COR | gsrt.FLAG_SH_GRAD),
                     lambda: sc.render_sharded_async(ubo, gsrt.MODE_COR | gsrt.FLAG_SH_GRAD)):
            with pytest.raises(gsrt.GsrtError) as e:
                call()
            assert e.value.status == gsrt.E_ARG and "SH_GRAD" in str(e.value)
            assert sc.render_sharded(ubo, gsrt.MODE_COR).tobytes() == plain.tobytes()


@pytest.fixture(params=["adaptive", "0", "1"])
def slot_knob(request, monkeypatch):
    if request.param != "adaptive":
        monkeypatch.setenv("GSRT_DEBUG_SLOT_STREAMS", request.param)
    return request.param


def test_frames_around_sh_gradient_frames_match_sync(ctx, slot_knob):
    """Plain, depth, feature, feature-gradient and SH-gradient frames queued without a sync in between match their
    synchronous renders, whatever the plain frames' slot-stream choice."""
    import torch

    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 20000, 11, True)
    n, C, W, H = len(o), 7, 64, 48
    ubo = ubo_of(W, H, 4, MOVED)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    sc.set_features(noise(n, C, 53))
    want_p = sc.render(ubo, gsrt.MODE_COR)[0]
    want_d = sc.render_depth(ubo)
    want_f = sc.render_features(ubo)
    G = noise(W * H, 4, 3, lo=0.0).reshape(H, W, 4)  # non-negative: see the comparison below
    Gf = noise(W * H, C, 4, lo=0.0).reshape(H, W, C)
    want_s = sc.sh_grad(ubo, G).astype(np.float64)
    want_g = sc.feature_grad(ubo, Gf).astype(np.float64)
    d_g, d_gf = torch.from_numpy(G).to("cuda:0"), torch.from_numpy(Gf).to("cuda:0")
    kinds = ["plain", "shgrad", "plain", "depth", "shgrad", "feat", "grad", "shgrad", "plain", "plain", "shgrad", "feat", "depth"]
    out = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in kinds]
    aux = [torch.zeros((n, 16, 3) if kd == "shgrad" else (n, C) if kd == "grad" else (H, W, C if kd == "feat" else 1),
                       dtype=torch.float32, device="cuda:0") for kd in kinds]
    for i, kd in enumerate(kinds):
        if kd == "plain":
            sc.render_async(ubo, gsrt.MODE_COR, d_rgba=out[i].data_ptr())
        elif kd == "depth":
            sc.render_depth_async(ubo, d_rgba=out[i].data_ptr(), d_depth=aux[i].data_ptr())
        elif kd == "feat":
            sc.render_features_async(ubo, d_rgba=out[i].data_ptr(), d_feat=aux[i].data_ptr())
        elif kd == "grad":
            sc.feature_grad_async(ubo, d_gf.data_ptr(), C, aux[i].data_ptr())
        else:
            sc.sh_grad_async(ubo, d_g.data_ptr(), aux[i].data_ptr())
            assert not ctx.slot_streams() and ctx.features_ptr() == 0 and ctx.depth_ptr() == 0
    ctx.synchronize()
    torch.cuda.synchronize()
    # two runs of one gradient differ by the order of their float atomic adds only. With G >= 0 every term of a feature
    # gradient, and of an SH gradient's coefficient 0 (Y_0 > 0), is non-negative: a sum of at most N = W H ns such terms
    # in any order lies within (N - 1) 2^-24 (1 + ..) of the exact sum, relative, so two orders differ by at most
    # N 2^-23 of the value
    rel = W * H * 4 * EPS
    for i, kd in enumerate(kinds):
        if kd == "plain":
            assert out[i].cpu().numpy().tobytes() == want_p.tobytes(), i
        elif kd == "depth":
            assert out[i].cpu().numpy().tobytes() == want_d[0].tobytes(), i
            assert aux[i].cpu().numpy()[..., 0].tobytes() == want_d[1].tobytes(), i
        elif kd == "feat":
            assert out[i].cpu().numpy().tobytes() == want_f[0].tobytes() and aux[i].cpu().numpy().tobytes() == want_f[1].tobytes(), i
        elif kd == "grad":
            assert (np.abs(aux[i].cpu().numpy() - want_g) <= rel * np.abs(want_g)).all(), i
        else:
            got = aux[i].cpu().numpy()
            assert (np.abs(got[:, 0, :] - want_s[:, 0, :]) <= rel * np.abs(want_s[:, 0, :])).all(), i
            assert np.isfinite(got).all(), i
    assert np.abs(want_s).max() > 0 and np.abs(want_g).max() > 0
    sc.close()


# ------------------------------------------------------------------------------------------------ 8: autograd
def test_autograd_descends_and_matches_sh_grad(ctx):
    """20 steps of plain descent from zeros on 0.5 |rgb - target|^2, the target rendered from a known table with
    |s| <= 0.02 (no clamp on the way: colours stay near 0.5). Step 1 / (16 0.75^2 max contributions): the Hessian's row
    sums are at most contributions[g] 0.75 16 0.75, since sum_g W_g <= 1 and |Y_q| <= 0.75. The backward's output is
    Scene.sh_grad of the same upstream gradient, both within the bound of the reference."""
    import torch

    from gsrt.autograd import render_colour

    model, _, (w, h, spp) = _cloud("sh3_1k")
    n = len(model[3])
    ubo = ubo_of(w, h, spp)
    sc = gsrt.Scene.from_model(ctx, *model, np.zeros((n, 16, 3), np.float32))
    try:
        sc.build_bvh()
        Wg = sample_weights(sc, ubo)
        B = basis_of(ctx, ubo)
        contrib = sc.contributions(ubo)
        assert contrib.max() > 0
        step = 1.0 / (16 * 0.75 ** 2 * float(contrib.max()))
        known = torch.from_numpy(small_table(n, 91)).to("cuda:0")
        with torch.no_grad():
            target = render_colour(sc, ubo, known).clone()
        table = torch.zeros((n, 16, 3), dtype=torch.float32, device="cuda:0", requires_grad=True)
        losses = []
        for it in range(20):
            rgba = render_colour(sc, ubo, table)
            loss = 0.5 * ((rgba[..., :3] - target[..., :3]).double() ** 2).sum()
            losses.append(float(loss.detach()))
            table.grad = None
            loss.backward()
            if it == 0:
                Gup = np.zeros((h, w, 4), np.float32)
                Gup[..., :3] = (rgba[..., :3] - target[..., :3]).detach().cpu().numpy()
                direct = sc.sh_grad(ubo, Gup).astype(np.float64)
                ref, bound = reference(Wg, B, np.ones((n, 3), bool), Gup)
                back = table.grad.cpu().numpy().astype(np.float64)
                assert (np.abs(back - ref) <= bound).all() and (np.abs(direct - ref) <= bound).all()
                assert (np.abs(back - direct) <= 2 * bound).all()
            with torch.no_grad():
                table -= step * table.grad
        assert all(b < a for a, b in zip(losses, losses[1:])), losses
        assert losses[-1] < 0.9 * losses[0]
    finally:
        sc.close()
