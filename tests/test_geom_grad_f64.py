"""The float64 geometry backward of tests/cor_f64_geom.py checked on the CPU, on the scene of test_grad_f64.py (the GPU
comparison, tests/test_geom_grad_gpu.py, holds the splat gradient frame and the projection's backward to it).

project() against cor_f64.Splats; model_chain() against central differences of project(); the two steps together against
central differences of <G, cor_f64.render> in centres and scales; slot 5 against cor_f64.gradients' opacity gradient; and
the conditioning kappa_g the GPU chain test's bound relies on; param_chain (cov3d back to the quaternion and the scales)
against central differences of cor_f64.covariance, and its power against the faults the glue of
gsrt.autograd.render_model could have (tests/test_model_grad_gpu.py holds every gradient of render_model to it).
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
    gs, ms = Q.scale_chain(r, s, ch.cov, mm.M2_cov)
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


# ---- the parameter chain, cov3d -> (rot, scale), and what tests/test_model_grad_gpu.py allows gsrt.autograd.render_model
EPS = 2.0 ** -24
GPU_CHAIN_OPS = 37  # tests/test_geom_grad_gpu.py's CHAIN_OPS (k_splat_grad_to_model); test_model_grad_gpu.py asserts it
KAPPA = 1.7  # the scene's largest kappa_g (test_scene_is_well_conditioned prints it; the GPU tests' bounds use it)
# The longest chain of rounded float32 operations in torch's backward of gsrt.autograd.model_covariance as it is written,
# from (rot, scale, the upstream gradient) to an output, a product counting one more than its two factors together:
#   R_ki 3 (two products at once, their sum, 1 - 2 (.); the doubling is exact), M = s R 4;
#   dL/dM_ki: einsum's backward, one matrix product per operand: M 4, the product 5, three terms 7, both operands' 8;
#   scale: sum_i dL/dM_ki R_ki: 8 + 3, the product 12, three terms 14;
#   rot:   dL/dR_ki = s_k dL/dM_ki 9, times the other factor of a quaternion product (exact input; doublings exact) 10,
#          and x (y, z alike) stands in ten such products (x y, x z and r x twice each, x x twice, both factors each
#          time), which autograd adds one after the other: 9 more, 19. r stands in six: 15.
N_TORCH = {"scale": 14, "rot": 19}


def model_tol(chain_ops=GPU_CHAIN_OPS):
    """render_model's cov3d and centre gradients against float64, in units of M2: one GPU splat gradient frame against
    float64 (the 1e-3 M the row tests hold; the chain is linear in the rows, so M2 of M carries it), and the chain
    kernel's bound plus as much again for float32 parameters that differ from the reference's in their last bits:
    test_render_model_backward's arithmetic with one frame instead of two."""
    return S.TOL + 2 * chain_ops * (1 + KAPPA) * EPS


def _fd_param_chain(r, s, dcov):
    """central differences of L = sum_g <dcov_g, cov6(F.covariance(r, s))_g>, one coordinate of every Gaussian at once (a
    Gaussian's cov3d depends on its own seven numbers only): (n, 3) for the scales, (n, 4) for the quaternion. L is a
    quadratic in each s_k, so its central difference is exact at any step and h = 1e-3 max_k s_k keeps the rounding of the
    difference (eps |L| / h) small against the smallest scale's M; in a quaternion entry L is a quartic: h = 1e-5."""
    def L(rr, ss):
        return (dcov * Q.cov6(F.covariance(rr, ss))).sum(1)

    gs, gq = np.zeros_like(s), np.zeros_like(r)
    hs = 1e-3 * s.max(1)
    for k in range(3):
        d = np.zeros_like(s)
        d[:, k] = hs
        gs[:, k] = (L(r, s + d) - L(r, s - d)) / (2 * hs)
    for k in range(4):
        d = np.zeros_like(r)
        d[:, k] = 1e-5
        gq[:, k] = (L(r + d, s) - L(r - d, s)) / 2e-5
    return gs, gq


@pytest.mark.parametrize("quats", ["unit", "scaled"])
def test_param_chain_matches_central_differences(quats):
    """param_chain against central differences of <dcov, cov6(F.covariance(r, s))> for random dcov, on the scene's own
    rotations and scales and with every quaternion scaled by a factor in [0.5, 1.5] (the radial part of the gradient, which
    a normalising parametrisation would not have). Bound: 1e-6 M, as test_model_chain_matches_central_differences."""
    _, r, s, _, _ = _model()
    rng = np.random.default_rng(53)
    if quats == "scaled":
        r = r * rng.uniform(0.5, 1.5, (S.N, 1))
    dcov = rng.uniform(-1.0, 1.0, (S.N, 6))
    got = Q.param_chain(r, s, dcov, np.abs(dcov))
    gs, gq = _fd_param_chain(r, s, dcov)
    ws = float((np.abs(gs - got.scale) / got.M_scale).max())
    wq = float((np.abs(gq - got.rot) / got.M_rot).max())
    print(f"param_chain ({quats} quaternions) against central differences: worst error / M = {ws:.3g} (scale), {wq:.3g} (rot)")
    assert (got.M_scale > 0).all() and (got.M_rot > 0).all()
    assert ws <= 1e-6 and wq <= 1e-6
    assert (np.abs(got.scale) <= got.M_scale * (1 + 1e-12)).all() and (np.abs(got.rot) <= got.M_rot * (1 + 1e-12)).all()
    # the scale part is the chain test_whole_gradient_matches_central_differences uses; its M takes R's entries whole
    g2, m2 = Q.scale_chain(r, s, dcov, np.abs(dcov))
    np.testing.assert_allclose(got.scale, g2, rtol=1e-12, atol=0)
    assert (m2 <= got.M_scale * (1 + 1e-12)).all()
    if quats == "scaled":  # the radial part is there: q . dL/dq = 2 <dL/dR, R - I> for R = I + a quadratic in q
        radial = (r * got.rot).sum(1)
        assert (np.abs(radial) > 1e-3 * (np.abs(r) * got.M_rot).sum(1)).sum() > S.N // 2


def wrong_param_chains(r, s, dcov, mcov):
    """the reference chain fed the faults the glue of render_model could have: name -> (scale, rot)"""
    conj = r * np.array([1.0, -1.0, -1.0, -1.0])
    off = np.array([1.0, 0.5, 0.5, 1.0, 0.5, 1.0])
    out = {}
    for name, d in (("slots xz and yy swapped", dcov[:, [0, 1, 3, 2, 4, 5]]), ("off-diagonals halved", dcov * off),
                    ("off-diagonals doubled", dcov / off)):
        w = Q.param_chain(r, s, d, mcov)
        out[name] = (w.scale, w.rot)
    w = Q.param_chain(conj, s, dcov, mcov)  # R of the conjugate is R transposed
    out["R transposed"] = (w.scale, w.rot * np.array([1.0, -1.0, -1.0, -1.0]))
    true = Q.param_chain(r, s, dcov, mcov)
    q2 = (r * r).sum(1, keepdims=True)
    out["radial part dropped"] = (true.scale, true.rot - r * (r * true.rot).sum(1, keepdims=True) / q2)
    return out


def test_param_chain_power():
    """In the manner of test_grad_f64.test_power: the float64 chain of CASES[0] (G as the GPU tests form it) fed each fault
    of wrong_param_chains differs from the true one by more than ten times test_model_grad_gpu.py's bound, (model_tol() +
    N_TORCH 2^-24) M, on a reached entry of scale.grad or rot.grad. Factors measured (error / bound, scale and rot): slots
    swapped 129 and 85; off-diagonals halved 35 and 27; doubled 70 and 53; R transposed 154 and 83; radial part dropped 0
    (it does not touch the scales) and 134: none needs another seed or case."""
    case = S.CASES[0]
    c, r, s, o, sh = _model()
    ubo = S.camera(*case)
    G = S.upstream(case, 4, 201 + case[3])  # test_grad_f64_gpu.reference's
    sg = Q.splat_gradients(ubo, c, r, s, o, sh, G_rgba=G)
    cov = Q.cov6(F.covariance(r, s))
    ch, mm = Q.model_chain(ubo, c, cov, sg.rows), Q.model_chain(ubo, c, cov, sg.M)
    true = Q.param_chain(r, s, ch.cov, mm.M2_cov)
    bs = (model_tol() + N_TORCH["scale"] * EPS) * true.M_scale
    bq = (model_tol() + N_TORCH["rot"] * EPS) * true.M_rot
    reached_s, reached_q = true.M_scale > 0, true.M_rot > 0
    assert reached_s.sum() > reached_s.size // 4 and reached_q.sum() > reached_q.size // 4
    for name, (ws, wq) in wrong_param_chains(r, s, ch.cov, mm.M2_cov).items():
        fs = float((np.abs(ws - true.scale)[reached_s] / bs[reached_s]).max())
        fq = float((np.abs(wq - true.rot)[reached_q] / bq[reached_q]).max())
        print(f"param chain with {name}: worst error / bound = {fs:.3g} (scale), {fq:.3g} (rot)")
        assert max(fs, fq) >= 10.0, name
        if name != "radial part dropped":
            assert fs >= 10.0 and fq >= 10.0, name


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
