"""The float64 geometry backward of tests/cor_f64_geom.py checked on the CPU, on the scene of test_grad_f64.py (the GPU
comparison, tests/test_geom_grad_gpu.py, holds the splat gradient frame and the projection's backward to it).

project() against cor_f64.Splats; model_chain() against central differences of project(); the two steps together against
central differences of <G, cor_f64.render> in centres and scales; slot 5 against cor_f64.gradients' opacity gradient; and
the conditioning kappa_g the GPU chain test's bound relies on.
"""
import numpy as np
import pytest

import cor_f64 as F
import cor_f64_geom as Q
import test_grad_f64 as S

FD_CASE = ("origin", 18, 18, 1)


def _model():
    c, r, s, o, sh = S.scene()
    return tuple(np.asarray(a, np.float64) for a in (c, r, s, o, sh))


def test_project_matches_splats():
    c, r, s, o, _ = _model()
    for case in (S.CASES[0], S.CASES[3], S.CASES[-1]):
        ubo = S.camera(*case)
        sp = F.Splats(F.Ubo(ubo), c, r, s, o)
        p = Q.project(ubo, c, Q.cov6(F.covariance(r, s)))
        assert np.array_equal(p.valid, sp.valid) and sp.valid.sum() > 100
        v = sp.valid
        for got, want in ((p.depth, sp.depth), (p.ppx, sp.ppx), (p.ppy, sp.ppy), (p.A, sp.ca), (p.B, sp.cb), (p.C, sp.cc)):
            np.testing.assert_allclose(got[v], want[v], rtol=1e-12, atol=0)
        # (n, 3, 3) covariances are taken as they are
        p3 = Q.project(ubo, c, F.covariance(r, s))
        assert np.array_equal(p3.A, p.A) and np.array_equal(p3.ppx, p.ppx)


def test_model_chain_matches_central_differences():
    """L = sum_g <f_g, (ppx, ppy, A, B, C)_g> with random f: a smooth function of each Gaussian's own nine numbers, so one
    pair of evaluations per coordinate differences every Gaussian at once. Steps: 1e-5 in a centre coordinate and 1e-5 of
    the Gaussian's mean variance in a cov3d entry. Bound: 1e-6 M2 (the h^2 and eps / h terms of float64 at these steps)."""
    c, r, s, o, _ = _model()
    ubo = S.camera("moved", 48, 32, 1)
    cov = Q.cov6(F.covariance(r, s))
    f = np.random.default_rng(31).uniform(-1.0, 1.0, (S.N, 5))
    got = Q.model_chain(ubo, c, cov, f)
    v = got.valid
    assert v.sum() > 100

    def L(cc, vv):
        p = Q.project(ubo, cc, vv)
        assert np.array_equal(p.valid, v)
        return np.stack([p.ppx, p.ppy, p.A, p.B, p.C], -1) * f  # per Gaussian, summed by the caller

    worst = 0.0
    for k in range(3):
        h = 1e-5
        d = np.zeros_like(c)
        d[:, k] = h
        fd = (L(c + d, cov) - L(c - d, cov)).sum(1) / (2 * h)
        err = np.abs(fd - got.center[:, k])[v] / got.M2_center[:, k][v]
        worst = max(worst, err.max())
    hs = 1e-5 * cov[:, [0, 3, 5]].mean(1)
    for k in range(6):
        d = np.zeros_like(cov)
        d[:, k] = hs
        fd = (L(c, cov + d) - L(c, cov - d)).sum(1) / (2 * hs)
        err = np.abs(fd - got.cov[:, k])[v] / got.M2_cov[:, k][v]
        worst = max(worst, err.max())
    print(f"model_chain against central differences: worst error / M2 = {worst:.3g}")
    assert worst <= 1e-6
    assert (np.abs(got.center) <= got.M2_center * (1 + 1e-12)).all() and (np.abs(got.cov) <= got.M2_cov * (1 + 1e-12)).all()
    assert not got.center[~v].any() and not got.cov[~v].any()


def _scale_chain(r, s, dcov, mcov):
    """dL/d(scale) from dL/d(cov3d) by hand: Sigma_ij = sum_k s_k^2 R_ki R_kj (cor_f64.covariance), so dSigma_ij / ds_k =
    2 s_k R_ki R_kj; a cov3d off-diagonal gradient already counts both places. Second result: the sum of absolute products."""
    q = np.asarray(r, np.float64)
    rr, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + rr * z), 2 * (x * z - rr * y)], -1),
                  np.stack([2 * (x * y - rr * z), 1 - 2 * (x * x + z * z), 2 * (y * z + rr * x)], -1),
                  np.stack([2 * (x * z + rr * y), 2 * (y * z - rr * x), 1 - 2 * (x * x + y * y)], -1)], -2)  # [n, k, i]
    # R's convention checked against covariance itself
    np.testing.assert_allclose(np.einsum("nk,nki,nkj->nij", s * s, R, R), F.covariance(r, s), rtol=1e-12, atol=1e-18)
    g, m = np.zeros_like(s), np.zeros_like(s)
    for e, (i, j) in enumerate(Q.COV_IJ):
        term = 2 * s * R[:, :, i] * R[:, :, j]  # (n, k)
        g += dcov[:, e, None] * term
        m += mcov[:, e, None] * np.abs(term)
    return g, m


def test_whole_gradient_matches_central_differences():
    """d<G, rgba>/d(centre) and /d(scale) by central differences of F.render for the eight Gaussians with the largest M
    (slots 0..4 summed), 18x18 at 1 spp, G zero on the float32-sensitive pixels. An entry's step starts at 1e-5 and is
    halved until the hit lists, their order and the clamp states at +h and -h are the base frame's (the digest), which is
    asserted. Bound: 1e-6 M, M the chain's sum of absolute products fed with splat_gradients' M (and through the scale
    chain's absolute products for a scale): the h^2 and eps / h terms of float64 at h ~ 1e-5."""
    c, r, s, o, sh = _model()
    ubo = S.camera(*FD_CASE)
    G = S.upstream(FD_CASE, 4, 41).astype(np.float64)
    sg = Q.splat_gradients(ubo, c, r, s, o, sh, G_rgba=G)
    base = F.gradients(ubo, c, r, s, o, sh)
    assert sg.digest == base.digest
    cov = Q.cov6(F.covariance(r, s))
    ch = Q.model_chain(ubo, c, cov, sg.rows)
    mm = Q.model_chain(ubo, c, cov, sg.M)
    gs, ms = _scale_chain(r, s, ch.cov, mm.M2_cov)
    picked = np.argsort(-sg.M[:, :5].sum(1))[:8]
    assert (sg.M[picked, :5].sum(1) > 0).all() and ch.valid[picked].all()
    worst = 0.0
    for g in picked:
        for what, k in [("center", k) for k in range(3)] + [("scale", k) for k in range(3)]:
            h = 1e-5
            for _ in range(12):
                side = []
                for sign in (-1.0, 1.0):
                    c1, s1 = c.copy(), s.copy()
                    (c1 if what == "center" else s1)[g, k] += sign * h
                    if F.gradients(ubo, c1, r, s1, o, sh).digest != base.digest:
                        break
                    side.append((G * F.render(ubo, c1, r, s1, o, sh)[0]).sum())
                if len(side) == 2:
                    break
                h /= 2
            assert len(side) == 2, (g, what, k, "no step keeps the hit sets")
            fd = (side[1] - side[0]) / (2 * h)
            want, M = (ch.center[g, k], mm.M2_center[g, k]) if what == "center" else (gs[g, k], ms[g, k])
            assert M > 0
            worst = max(worst, abs(fd - want) / M)
            assert abs(fd - want) <= 1e-6 * M, (int(g), what, k, h, fd, want, M)
    print(f"whole gradient against central differences: worst error / M = {worst:.3g}")


@pytest.mark.parametrize("with_sh", [True, False])
def test_slot5_is_the_opacity_gradient(with_sh):
    c, r, s, o, sh = _model()
    case = S.CASES[0]
    ubo = S.camera(*case)
    G = S.upstream(case, 4, 42, with_sh)
    rows = sh if with_sh else None
    sg = Q.splat_gradients(ubo, c, r, s, o, rows, G_rgba=G)
    ref = F.gradients(ubo, c, r, s, o, rows, G_rgba=G)
    assert sg.digest == ref.digest and np.array_equal(sg.near, ref.near)
    np.testing.assert_allclose(sg.rows[:, 5], ref.opacity, rtol=1e-12, atol=0)
    np.testing.assert_allclose(sg.M[:, 5], ref.M_opacity, rtol=1e-12, atol=0)
    assert not sg.rows[:, 6:].any() and not sg.M[:, 6:].any()
    assert (np.abs(sg.rows) <= sg.M * (1 + 1e-12)).all()
    assert ((sg.M[:, :5] > 0).sum(0) > S.N // 4).all()


@pytest.mark.parametrize("cam", sorted(S.CAMERAS))
def test_scene_is_well_conditioned(cam):
    """kappa_g = v00 v11 / det <= 1e4 on every valid splat, under both cameras and both frame sizes: the bound of the GPU
    chain test grows with it"""
    c, r, s, _, _ = _model()
    for case in S.CASES:
        if case[0] != cam:
            continue
        ch = Q.model_chain(S.camera(*case), c, Q.cov6(F.covariance(r, s)), np.zeros((S.N, 8)))
        print(f"{case}: {ch.valid.sum()} valid splats, largest kappa {ch.kappa.max():.4g}")
        assert ch.valid.sum() > 100 and (ch.kappa[ch.valid] >= 1.0).all()
        assert (ch.kappa[ch.valid] <= 1e4).all()
