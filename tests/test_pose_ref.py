"""The float64 pose backward of tests/cor_f64_pose.py checked on the CPU (the GPU comparison, tests/test_pose_grad_gpu.py,
holds gsrt_pose_grad to it): pose_chain against central differences of the projection and of the float64 renderer's loss,
the translation identity that ties it to model_chain, the twist helpers, and the power of the GPU test's bound against four
faults a pose kernel could have, on the GPU test's own cases (tests/pose_cases.py).
"""
import numpy as np
import pytest

import cor_f64 as F
import cor_f64_depth as D
import cor_f64_geom as Q
import cor_f64_pose as PQ
import pose_cases as PC
import test_depth_grad_f64 as SD
import test_grad_f64 as S

REAL_CASES = [S.CASES[0], S.CASES[3], S.CASES[-1]]  # test_geom_grad_gpu.test_chain_kernel_matches_f64's three


def ubo64(ubo):
    """the ubo record with float64 fields, so that a model-view can be stepped by less than a float32 ulp"""
    dt = np.dtype([(k, np.float64 if ubo.dtype[k].base == np.float32 else ubo.dtype[k].base, ubo.dtype[k].shape)
                   for k in ubo.dtype.names])
    out = np.zeros(1, dt)
    for k in ubo.dtype.names:
        out[k] = ubo[k]
    return out


def stepped(ubo, r, c, h):
    u = ubo64(ubo)
    u["model_view"][0][c * 4 + r] += h
    return u


@pytest.mark.parametrize("depth", [False, True], ids=["plain", "depth"])
@pytest.mark.parametrize("cam", ["affine", "nonaffine"])
def test_pose_chain_matches_central_differences(cam, depth):
    """All 16 entries of MV, of the linear functional sum_g rows_g . (ppx, ppy, A, B, C[, depth])(MV) through
    cor_f64_geom.project with only MV perturbed. Step 1e-6; bound 1e-6 M (the h^2 and eps / h terms of float64)."""
    ubo = PC.camera() if cam == "affine" else PC.nonaffine_camera()
    params, _, rows, behind = PC.synthetic(300, 5, ubo)
    c, cov, rows = params[:, :3].astype(np.float64), params[:, 4:10].astype(np.float64), rows.astype(np.float64)
    ref = PQ.pose_chain(ubo, c, cov, rows, depth)
    assert not ref.valid[behind].any() and ref.valid.sum() >= 240
    MV = PQ.mat(ubo["model_view"][0])
    worst = 0.0
    for r in range(4):
        for cc in range(4):
            h = 1e-6
            d = np.zeros((4, 4))
            d[r, cc] = h
            fd = (PQ.linear_functional(ubo, MV + d, c, cov, rows, depth) -
                  PQ.linear_functional(ubo, MV - d, c, cov, rows, depth)) / (2 * h)
            if ref.M[r, cc] == 0:  # the bottom row under the plain perspective matrix: nothing reaches it
                assert r == 3 and cam == "affine" and fd == 0 and ref.G[r, cc] == 0
                continue
            worst = max(worst, abs(fd - ref.G[r, cc]) / ref.M[r, cc])
    print(f"pose_chain {cam} depth={depth} against central differences: worst error / M = {worst:.3g}")
    assert worst <= 1e-6
    assert (np.abs(ref.G) <= ref.M * (1 + 1e-12)).all() and np.allclose(ref.Mg.sum(0), ref.M)


def test_whole_pose_gradient_matches_central_differences():
    """d<G, rgba>/dMV by central differences of F.render on a scene without SH rows (its colour is constant, so the
    model_view_inverse partial is zero and pose_chain is the whole gradient): the first 40 Gaussians of test_grad_f64's
    scene at 32x32, 1 spp, G zero on the float32-sensitive pixels; model_view stepped, model_view_inverse held. A step
    starts at 1e-5 and is halved until the hit lists, their order and the clamp states at +h and -h are the base frame's
    (the digest). Bound: 1e-6 M, M the chain fed with splat_gradients' M."""
    c, r, s, o, _ = (np.asarray(a[:40], np.float64) for a in S.scene())
    ubo = S.camera("origin", 32, 32, 1)
    near = F.render(ubo, c, r, s, o)[1]
    G = S.noise(32 * 32, 4, 77).reshape(32, 32, 4).astype(np.float64) * ~near[:, :, None]
    sg = Q.splat_gradients(ubo, c, r, s, o, None, G_rgba=G)
    base = F.gradients(ubo, c, r, s, o, None, G_rgba=G)
    assert sg.digest == base.digest
    cov = Q.cov6(F.covariance(r, s))
    ref = PQ.pose_chain(ubo, c, cov, sg.rows)
    M = PQ.pose_chain(ubo, c, cov, sg.M).M
    assert ref.valid.sum() >= 20 and np.abs(ref.G).max() > 0
    worst = 0.0
    for rr in range(4):
        for cc in range(4):
            h = 1e-5
            for _ in range(14):
                side = []
                for sign in (-1.0, 1.0):
                    u = stepped(ubo, rr, cc, sign * h)
                    if F.gradients(u, c, r, s, o, None, G_rgba=G).digest != base.digest:
                        break
                    side.append((G * F.render(u, c, r, s, o)[0]).sum())
                if len(side) == 2:
                    break
                h /= 2
            assert len(side) == 2, (rr, cc, "no step keeps the hit sets")
            fd = (side[1] - side[0]) / (2 * h)
            if M[rr, cc] == 0:  # the bottom row under the plain perspective matrix
                assert rr == 3 and fd == 0 and ref.G[rr, cc] == 0
                continue
            worst = max(worst, abs(fd - ref.G[rr, cc]) / M[rr, cc])
            assert abs(fd - ref.G[rr, cc]) <= 1e-6 * M[rr, cc], (rr, cc, h, fd, ref.G[rr, cc], M[rr, cc])
    print(f"whole pose gradient against central differences: worst error / M = {worst:.3g}")


def test_translation_column_is_the_summed_centre_gradient():
    """For an affine MV a world translation of every centre is a camera translation: sum_g grad_centre_g =
    MV_3x3^T G[0:3, 3], with model_chain's centres (plain rows)."""
    ubo = PC.camera()
    params, _, rows, _ = PC.synthetic(500, 9)
    c, cov, rows = params[:, :3].astype(np.float64), params[:, 4:10].astype(np.float64), rows.astype(np.float64)
    ref = PQ.pose_chain(ubo, c, cov, rows)
    mc = Q.model_chain(ubo, c, cov, rows)
    MV = PQ.mat(ubo["model_view"][0])
    np.testing.assert_allclose(mc.center.sum(0), MV[:3, :3].T @ ref.G[:3, 3], rtol=0, atol=1e-12 * mc.M2_center.sum(0).max())


def test_twist_and_retraction():
    """twist is the derivative of L(exp(xi^) MV) at 0 for a linear L = <G, .>; apply_twist inverts itself, keeps
    MV MVinv = I, and log_twist recovers the twist"""
    rng = np.random.default_rng(3)
    MV, G = PQ.mat(PC.camera()["model_view"][0]), rng.normal(size=(4, 4))
    g = PQ.twist(MV, G)
    for k in range(6):
        e = np.zeros(6)
        e[k] = 1e-6
        fd = ((G * PQ.apply_twist(MV, np.linalg.inv(MV), e)[0]).sum() - (G * PQ.apply_twist(MV, np.linalg.inv(MV), -e)[0]).sum()) / 2e-6
        assert abs(fd - g[k]) <= 1e-8 * np.abs(G).sum() * np.abs(MV).max()
    for xi in (np.array([0.3, -0.2, 0.1, 0.0, 0.0, 0.0]), np.array([0.1, 0.2, -0.3, 0.4, -0.5, 0.6]),
               np.array([0.0, 0.0, 0.0, 1e-8, 0.0, 0.0]), np.array([0.1, 0.0, 0.2, 0.0, 3.0, 0.0])):
        A, Ai = PQ.apply_twist(MV, np.linalg.inv(MV), xi)
        np.testing.assert_allclose(A @ Ai, np.eye(4), atol=1e-12)
        np.testing.assert_allclose(PQ.log_twist(A @ np.linalg.inv(MV)), xi, atol=1e-10)
        R = PQ.expm(PQ.hat(xi))[:3, :3]
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-12)


# ---- the power of the GPU test's bound -------------------------------------------------------------------------------

def misses(ubo, params, rows, depth, fault):
    """the largest |faulty - true| / bound over the 16 entries: how far a kernel with that fault would miss the bound"""
    G, B, _ = PC.reference(ubo, params, rows, depth)
    Gf = PC.reference(ubo, params, rows, depth, fault)[0]
    reached = B > 0  # an entry nothing reaches (the bottom row under the plain perspective matrix) must stay 0
    if (Gf[~reached] != 0).any():
        return np.inf
    return float((np.abs(Gf - G)[reached] / B[reached]).max())


@pytest.mark.parametrize("n,depth", PC.seam_cases(), ids=lambda v: str(v))
def test_bound_sees_the_faults_on_the_seam_cases(n, depth):
    """the direct T term dropped, G transposed and, in the depth form, slot 6 ignored: each misses the bound at least ten
    times over on every seam case of the GPU test"""
    ubo = PC.camera()
    params, _, rows, _ = PC.synthetic(n, 100 + n % 97)
    for fault in ("direct", "transpose") + (("slot6",) if depth else ()):
        ratio = misses(ubo, params, rows, depth, fault)
        print(f"seam n={n} depth={depth} fault {fault}: misses the bound {ratio:.3g} times over")
        assert ratio >= 10.0, (fault, ratio)


@pytest.mark.parametrize("depth", [False, True], ids=["plain", "depth"])
def test_bound_sees_the_faults_on_the_nonaffine_case(depth):
    """all four, the bottom row dropped among them: under a non-affine MV the bottom row's gradient is not zero"""
    ubo = PC.nonaffine_camera()
    params, _, rows, _ = PC.synthetic(777, 21, ubo)
    for fault in ("direct", "transpose", "bottom") + (("slot6",) if depth else ()):
        ratio = misses(ubo, params, rows, depth, fault)
        print(f"non-affine depth={depth} fault {fault}: misses the bound {ratio:.3g} times over")
        assert ratio >= 10.0, (fault, ratio)


@pytest.mark.parametrize("case", REAL_CASES, ids=lambda c: "%s-%dx%d-spp%d" % c)
def test_bound_sees_the_faults_on_real_rows(case):
    """the float64 rows of the frames whose float32 rows the GPU test takes from Scene.splat_grad and splat_depth_grad"""
    c, r, s, o, sh = S.scene()
    ubo = S.camera(*case)
    G = S.upstream(case, 4, 201 + case[3], True)
    Gd = SD.upstream_depth(case, 301 + case[3], True)
    params = np.zeros((S.N, 12), np.float32)
    params[:, :3], params[:, 3], params[:, 4:10] = c, o, Q.cov6(F.covariance(r, s))
    plain = Q.splat_gradients(ubo, c, r, s, o, sh, G_rgba=G).rows.astype(np.float32)
    deep = D.depth_gradients(ubo, c, r, s, o, sh, G_rgba=G, G_depth=Gd).rows.astype(np.float32)
    for depth, rows in ((False, plain), (True, deep)):
        for fault in ("direct", "transpose") + (("slot6",) if depth else ()):
            ratio = misses(ubo, params, rows, depth, fault)
            print(f"real rows {case} depth={depth} fault {fault}: misses the bound {ratio:.3g} times over")
            assert ratio >= 10.0, (fault, ratio)
