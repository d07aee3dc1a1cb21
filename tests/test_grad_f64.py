"""The float64 backward of tests/cor_f64.py (F.gradients) checked on the CPU, and the scene the GPU comparison uses
(tests/test_grad_f64_gpu.py holds the three gradient kernels to F.gradients on it).

F.gradients is derived from the blend's definition, so these tests pin it from four sides: closed forms of a two-Gaussian
ray, the adjoint identities of the two linear backwards against F.render, central differences of F.render in single
opacities, and the conditions the scene must meet for the comparison to reach the clamps: alpha clamped at 0.99 behind
another hit, and a Gaussian's colour channel clamped at 0 on some rays and open on others. test_power shows that a
backward without the clamps' selects misses the GPU tests' tolerance on this scene by more than a factor of ten.
"""
import os

import numpy as np
import pytest

import cor_f64 as F
import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-3  # the GPU tests' bound per table entry, in units of the entry's magnitude M
N, SEED, CLAMPED_SHARE = 300, 107, 0.7
CAMERAS = {"origin": ((0, 0, 0), (0, 0, -1)), "moved": ((0.05, -0.03, 0.1), (0.02, 0, -1))}
# (camera, width, height, spp) of every GPU comparison: 4 spp in the wave, 3 spp as passes, 1 spp, a ragged frame
CASES = [(cam, 48, 32, spp) for cam in CAMERAS for spp in (4, 3, 1)] + [("origin", 18, 18, 4)]
_CACHE = {}


def scene():
    """The first N Gaussians of the sh3_1k cloud; opacity 1 on CLAMPED_SHARE of them (alpha clamps near their centres,
    mostly behind other hits), an SH table whose colours cross 0 with the ray direction: (c, r, s, o, sh), float32."""
    if "scene" not in _CACHE:
        z = np.load(os.path.join(GOLD, "cor_sh3_1k.npz"))
        c, r, s, o = (np.ascontiguousarray(z[k][:N], np.float32) for k in ("center", "rot", "scale", "opacity"))
        rng = np.random.default_rng(SEED)
        o[rng.random(N) < CLAMPED_SHARE] = 1.0
        sh = rng.uniform(-0.5, 0.5, (N, 16, 3)).astype(np.float32)
        sh[:, 0, :] = rng.uniform(-2.5, 1.0, (N, 3)).astype(np.float32)
        _CACHE["scene"] = (c, r, s, o, sh)
    return _CACHE["scene"]


def camera(cam, w, h, spp):
    return O.make_ubo(O.lookat(*CAMERAS[cam]), 60.0, w, h, 1.0, spp, 16)


def noise(n, channels, seed, lo=-3.0, hi=3.0):
    return np.random.default_rng(seed).uniform(lo, hi, (n, channels)).astype(np.float32)


def sensitive(case, with_sh=True):
    """the case's result without an upstream gradient: the float32-sensitive pixels and the event counts, computed once"""
    key = ("near", case, with_sh)
    if key not in _CACHE:
        c, r, s, o, sh = scene()
        _CACHE[key] = F.gradients(camera(*case), c, r, s, o, sh if with_sh else None)
    return _CACHE[key]


def upstream(case, channels, seed, with_sh=True):
    """G (h, w, channels) float32: noise, zero on the float32-sensitive pixels"""
    _, w, h, _ = case
    G = noise(w * h, channels, seed).reshape(h, w, channels)
    G[sensitive(case, with_sh).near] = 0.0
    return G


# ------------------------------------------------------------------------------------------------ 1: by hand
def test_two_gaussians_by_hand():
    """Two isotropic Gaussians on the optical axis, 33x33 at fovy 90 and 1 spp (f = 16.5 px, both project to (16.5,
    16.5)): the front one (depth 4, sigma 2, opacity 1) clamps at the centre pixel A and is open at pixel B, 14 columns
    to the right; the back one (depth 6, sigma 3, opacity 0.6) is open at both. SH rows with coefficient 0 only; one
    channel of each is clamped at 0. G is non-zero at A and B only."""
    ubo = O.make_ubo(O.lookat((0, 0, 0), (0, 0, -1)), 90.0, 33, 33, 1.0, 1, 16)
    sh = np.zeros((2, 16, 3))
    sh[0, 0], sh[1, 0] = (-2.0, 1.0, 0.5), (1.0, -3.0, 0.2)
    col = np.maximum(0.0, 0.5 + F.SH_C0 * sh[:, 0, :])
    open_ch = 0.5 + F.SH_C0 * sh[:, 0, :] > 0
    assert open_ch.tolist() == [[False, True, True], [True, False, True]]
    G = np.zeros((33, 33, 4))
    Gf = np.zeros((33, 33, 2))
    A, B = (16, 16), (16, 30)  # (row, column)
    G[A], G[B] = (0.7, -1.1, 0.4, 1.3), (-0.9, 0.6, 1.2, -0.8)
    Gf[A], Gf[B] = (0.5, -2.0), (1.5, 0.25)
    got = F.gradients(ubo, [[0, 0, -4], [0, 0, -6]], [[1, 0, 0, 0]] * 2, [[2.0] * 3, [3.0] * 3], [1.0, 0.6], sh,
                      G_rgba=G, G_feat=Gf)
    jx, jy = F.jitter(int(ubo["random_seed"][0]), 1)[0]
    v = [(16.5 * 2.0 / 4.0) ** 2 + 0.3, (16.5 * 3.0 / 6.0) ** 2 + 0.3]
    want_o, want_sh0, want_f = np.zeros(2), np.zeros((2, 3)), np.zeros((2, 2))
    for (y, x), clamped in ((A, True), (B, False)):
        dx, dy = x + jx - 16.5, y + jy - 16.5
        e = [np.exp(-0.5 * (dx * dx + dy * dy) / v[k]) for k in range(2)]
        assert (1.0 * e[0] >= 0.99) == clamped
        a1, a2 = min(e[0], 0.99), 0.6 * e[1]
        g = G[y, x]
        # rgb = col1 a1 + col2 a2 (1 - a1), alpha = 1 - (1 - a1)(1 - a2)
        if not clamped:
            want_o[0] += (g[:3] @ (col[0] - col[1] * a2) + g[3] * (1 - a2)) * e[0]
        want_o[1] += (g[:3] @ ((1 - a1) * col[1]) + g[3] * (1 - a1)) * e[1]
        w = [a1, a2 * (1 - a1)]
        for k in range(2):
            want_sh0[k] += F.SH_C0 * w[k] * g[:3] * open_ch[k]
            want_f[k] += w[k] * Gf[y, x]
    assert not got.near[A] and not got.near[B]
    assert got.counts["clamped"] >= 1 and got.counts["clamped_behind"] == 0 and got.counts["hits"] > 2
    np.testing.assert_allclose(got.opacity, want_o, rtol=1e-12)
    np.testing.assert_allclose(got.sh[:, 0, :], want_sh0, rtol=1e-12, atol=0)
    np.testing.assert_allclose(got.feat, want_f, rtol=1e-12)
    assert (got.sh[0, :, 0] == 0).all() and (got.sh[1, :, 1] == 0).all()  # the clamped channels
    # the other coefficients: the term of coefficient 0 times Y_q / Y_0 of the one pixel that reaches them. With G at B
    # alone, x_ndc = 2 (30 + jx) / 33 - 1, y_ndc likewise from row 16, direction (x_ndc, -y_ndc, -1) normalised: the
    # projection's P11 is -1 at fovy 90 (rows run downwards)
    assert np.asarray(ubo["projection"][0]).reshape(4, 4)[1, 1] == -1.0
    G[A] = 0.0
    at_b = F.gradients(ubo, [[0, 0, -4], [0, 0, -6]], [[1, 0, 0, 0]] * 2, [[2.0] * 3, [3.0] * 3], [1.0, 0.6], sh, G_rgba=G)
    d = np.array([2 * (30 + jx) / 33 - 1, -(2 * (16 + jy) / 33 - 1), -1.0])
    d /= np.linalg.norm(d)
    np.testing.assert_allclose(at_b.sh[0, 3, 1:], at_b.sh[0, 0, 1:] * (-F.SH_C1 * d[0]) / F.SH_C0, rtol=1e-12)
    np.testing.assert_allclose(at_b.sh[0, 2, 1:], at_b.sh[0, 0, 1:] * (F.SH_C1 * d[2]) / F.SH_C0, rtol=1e-12)
    np.testing.assert_allclose(at_b.sh[1, 1, 0], at_b.sh[1, 0, 0] * (-F.SH_C1 * d[1]) / F.SH_C0, rtol=1e-12)
    # and the magnitudes bound the values
    assert (np.abs(got.opacity) <= got.M_opacity).all() and (np.abs(got.sh) <= got.M_sh).all()


# ------------------------------------------------------------------------------------------------ 2: adjoint identities
SMALL = ("origin", 18, 18, 4)


def test_feature_adjoint_identity():
    """<G, feat(table)> = <grad_feat, table>: the feature frame is linear in the table. The frame is F.render's colour
    of rows that encode three non-negative features (test_features_match_f64)."""
    c, r, s, o, _ = scene()
    ubo = camera(*SMALL)
    table = np.random.default_rng(11).uniform(0.0, 8.0, (N, 3))
    rows = np.zeros((N, 16, 3))
    rows[:, 0, :] = (table - 0.5) / F.SH_C0
    G = noise(18 * 18, 3, 12).reshape(18, 18, 3).astype(np.float64)
    feat = F.render(ubo, c, r, s, o, rows)[0][..., :3]
    got = F.gradients(ubo, c, r, s, o, G_feat=G)
    lhs, rhs = (G * feat).sum(), (got.feat * table).sum()
    assert abs(lhs - rhs) <= 1e-10 * (got.M_feat * table).sum()
    assert (got.M_feat * table).sum() > 1.0


def test_sh_adjoint_identity():
    """<G, rgba(sh + d) - rgba(sh)> = <grad_sh, d> while no colour changes sign. d_q = 1e-3 s_q u with |u| <= 1/2 moves a
    channel by less than col_rel = 1e-3 times the size of its terms, so every pixel where a sign can change is in `near`,
    where G is zero; that the signs G can see did not change is checked: grad_sh depends on the table through them only."""
    c, r, s, o, sh = scene()
    ubo = camera("origin", 18, 18, 1)
    rel = 1e-3
    near = F.gradients(ubo, c, r, s, o, sh, col_rel=rel).near
    assert 0.0 < near.mean() < 0.8
    G = noise(18 * 18, 4, 13).reshape(18, 18, 4).astype(np.float64)
    G[near] = 0.0
    sh64 = sh.astype(np.float64)
    d = rel * sh64 * np.random.default_rng(14).uniform(-0.5, 0.5, sh64.shape)
    base = F.gradients(ubo, c, r, s, o, sh64, G_rgba=G, col_rel=rel)
    moved = F.gradients(ubo, c, r, s, o, sh64 + d, G_rgba=G, col_rel=rel)
    assert np.array_equal(base.sh, moved.sh) and base.counts["channels_clamped"] != moved.counts["channels_clamped"]
    diff = F.render(ubo, c, r, s, o, sh64 + d)[0] - F.render(ubo, c, r, s, o, sh64)[0]
    lhs, rhs = (G * diff).sum(), (base.sh * d).sum()
    size = (base.M_sh * np.abs(d)).sum()
    assert abs(lhs - rhs) <= 1e-10 * size
    assert abs(rhs) > 1e-4 * size


# ------------------------------------------------------------------------------------------------ 3: central differences
def test_opacity_central_differences():
    """d<G, rgba>/d o_g by central differences of F.render, step 1e-6, for eight Gaussians, first those with a clamped hit
    in the frame (up to four), then others, each the largest by M: within 1e-6 M. An entry counts only if the hit lists and clamp states at o - h, o and o + h are the
    same (the digest); at most one may be left out."""
    case = ("origin", 18, 18, 1)
    c, r, s, o, sh = scene()
    ubo = camera(*case)
    o64 = o.astype(np.float64)
    G = upstream(case, 4, 15).astype(np.float64)
    got = F.gradients(ubo, c, r, s, o64, sh, G_rgba=G)
    where = sensitive(case)
    by_size = np.argsort(-got.M_opacity)
    picked = [g for g in by_size if where.gauss_clamped[g]][:4]
    assert len(picked) >= 2 and (o64[picked] == 1.0).all()
    picked += [g for g in by_size if not where.gauss_clamped[g]][:8 - len(picked)]
    h = 1e-6
    checked = 0
    for g in picked:
        side = []
        for sign in (-1.0, 1.0):
            o1 = o64.copy()
            o1[g] += sign * h
            side.append(F.render(ubo, c, r, s, o1, sh)[0])
            if F.gradients(ubo, c, r, s, o1, sh).digest != got.digest:
                break
        else:
            checked += 1
            fd = (G * (side[1] - side[0])).sum() / (2 * h)
            assert got.M_opacity[g] > 0.1
            assert abs(fd - got.opacity[g]) <= 1e-6 * got.M_opacity[g], (g, fd, got.opacity[g], got.M_opacity[g])
    assert checked >= 7


# ------------------------------------------------------------------------------------------------ 4: the scene
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%dx%d-spp%d" % c)
def test_scene_conditions(case):
    """What the GPU comparison needs of every frame it renders. mean_alpha is the mean of the frame's alpha channel."""
    res = sensitive(case)
    cn = res.counts
    print(f"{case}: sensitive {res.near.mean():.2%}; {cn}")
    assert res.near.mean() <= 0.10
    assert cn["clamped_behind"] >= 20
    assert cn["mixed_pairs"] >= 100
    assert cn["stopped_rays"] >= 1
    assert cn["mean_alpha"] > 0.5
    bare = sensitive(case, with_sh=False)  # the frame without SH rows: the same hits, no colour decisions
    assert bare.near.mean() <= res.near.mean() and bare.counts["clamped_behind"] == cn["clamped_behind"]


# ------------------------------------------------------------------------------------------------ 5: power
def test_power():
    """A backward that treats every hit as open and every channel as unclamped differs from the true one by more than ten
    times the GPU tests' tolerance on at least 20 opacities and 50 SH coefficients: the comparison can fail for the bugs
    it is there to catch. G as the GPU tests form it, zero on the sensitive pixels."""
    case = CASES[0]
    c, r, s, o, sh = scene()
    G = upstream(case, 4, 16)
    true = F.gradients(camera(*case), c, r, s, o, sh, G_rgba=G)
    wrong = F.gradients(camera(*case), c, r, s, o, sh, G_rgba=G, clamp_selects=False)
    off_o = np.abs(wrong.opacity - true.opacity) > 10 * TOL * true.M_opacity
    off_sh = np.abs(wrong.sh - true.sh) > 10 * TOL * true.M_sh
    print(f"without the selects: {off_o.sum()} of {N} opacities and {off_sh.sum()} of {N * 48} SH entries off by > 10 tol")
    assert off_o.sum() >= 20 and off_sh.sum() >= 50
    assert true.digest == wrong.digest
