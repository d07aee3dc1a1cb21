"""The geometry backward on the GPU against the float64 one of tests/cor_f64_geom.py (checked on the CPU by
tests/test_geom_grad_f64.py): the splat gradient frame (gsrt_render_splat_grad), the projection's backward
(gsrt_splat_grad_to_model), Scene.geometry_grad, accumulate, and gsrt.autograd.render_model.

Scene, cameras, upstream gradients and frames are those of tests/test_grad_f64_gpu.py (300 Gaussians, frames of at most
48x32 pixels, 1, 3 and 4 spp), whose conditions (alphas clamped behind other hits, stops, mixed clamps) are asserted on the
CPU in tests/test_grad_f64.py; its reference cache, its `hold` (every entry within 1e-3 M, entries nothing reaches +0, the
worst ratio printed and appended to COR_F64_REPORT) and its frame_checks are used as they are. G is zero on the
float32-sensitive pixels. Measured ratios: DESIGN.md section 5.
"""
import numpy as np
import pytest

import cor_f64 as F
import cor_f64_geom as Q
import gsrt
import test_grad_f64 as S
import test_grad_f64_gpu as TG
from test_features_gpu import u32

pytestmark = pytest.mark.gpu

CASES = TG.CASES
# the longest chain of rounded float32 operations from the kernel's inputs to one of its outputs, counted in
# k_splat_grad_to_model as it is written (cor_chain_grad's header in gsrt_project.hpp lists the steps to dL/dt): t 4,
# 1 / depth 1, its square 1, j02 1, T0 1, u0 3, v00 4, det 1, 1 / det 1, A 1, Q G 2, W 2, dL/dT0 2, dL/dj02 3,
# dL/d(1 / depth) 4, dL/dt2 1, + the ppx, ppy part 1, MV^T dL/dt 4
CHAIN_OPS = 37
EPS = 2.0 ** -24
_REF = {}


def reference(case, with_sh):
    """TG.reference's G and frame, and the float64 splat rows of that G; computed once per case"""
    key = (case, with_sh)
    if key not in _REF:
        c, r, s, o, sh = S.scene()
        G, ref, want = TG.reference(case, with_sh)
        sg = Q.splat_gradients(TG.camera(case), c, r, s, o, sh if with_sh else None, G_rgba=G)
        assert sg.digest == ref.digest and np.array_equal(sg.near, ref.near)
        _REF[key] = (G, sg, want)
    return _REF[key]


def rows_check(label, ctx, case, with_sh):
    c, r, s, o, sh = S.scene()
    G, sg, want = reference(case, with_sh)
    ubo = TG.camera(case)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh if with_sh else None)
    try:
        sc.build_bvh()
        got = sc.splat_grad(ubo, G)
        TG.frame_checks(ctx, sc, ubo, case, want)
    finally:
        sc.close()
    assert got.shape == (S.N, 8) and got.dtype == np.float32
    assert not u32(got[:, 6:]).any()  # slots 6 and 7: all bits zero
    TG.hold(label, case, sg.near, got[:, :6], sg.rows[:, :6], sg.M[:, :6])


@CASES
def test_rows_with_sh_match_f64(ctx, case):
    rows_check("splat-grad SH", ctx, case, True)


@CASES
def test_rows_without_sh_match_f64(ctx, case):
    rows_check("splat-grad colour 1", ctx, case, False)


@pytest.mark.parametrize("case", [S.CASES[0], S.CASES[3], S.CASES[-1]], ids=lambda c: "%s-%dx%d-spp%d" % c)
def test_chain_kernel_matches_f64(ctx, case):
    """Scene.model_grad of the float32 reference rows against model_chain of those same rows and the scene's own float32
    parameters (Scene.download). Per entry |got - ref| <= CHAIN_OPS (1 + kappa_g) 2^-24 M2: every one of the chain's
    CHAIN_OPS operations rounds a value that M2 bounds by half an ulp, and the recomputed conic carries the forward's
    rounding amplified by kappa_g = v00 v11 / det (at most 1.7 on this scene, test_geom_grad_f64.py). Six Gaussians are
    moved behind the camera and given rows of ones: invalid splats get +0."""
    c, r, s, o, _ = S.scene()
    sg = reference(case, True)[1]
    ubo = TG.camera(case)
    behind = np.arange(0, S.N, S.N // 6)[:6]
    c = c.copy()
    mv = F.Ubo(ubo).MV
    c[behind] = (np.linalg.inv(mv) @ np.array([0.3, -0.2, 2.5, 1.0]))[:3].astype(np.float32)  # view z > 0: depth < 0
    rows = sg.rows.astype(np.float32)
    rows[behind] = 1.0
    sc = gsrt.Scene.from_model(ctx, c, r, s, o)
    try:
        sc.build_bvh()
        params, _ = sc.download()
        gc, gv = sc.model_grad(ubo, rows)
    finally:
        sc.close()
    ref = Q.model_chain(ubo, params[:, :3].astype(np.float64), params[:, 4:10].astype(np.float64), rows.astype(np.float64))
    assert not ref.valid[behind].any() and ref.valid.sum() == S.N - 6
    assert gc.shape == (S.N, 3) and gv.shape == (S.N, 6) and np.isfinite(gc).all() and np.isfinite(gv).all()
    assert not u32(gc[behind]).any() and not u32(gv[behind]).any()
    worst = 0.0
    for name, got, want, M2 in (("centre", gc, ref.center, ref.M2_center), ("cov", gv, ref.cov, ref.M2_cov)):
        bound = CHAIN_OPS * (1.0 + ref.kappa[:, None]) * EPS * M2
        err = np.abs(got.astype(np.float64) - want)
        reached = M2 > 0
        assert reached.sum() > M2.size // 4
        ratio = float((err[reached] / bound[reached]).max())
        worst = max(worst, ratio)
        print(f"model-grad {name} {case}: worst error / (N (1 + kappa) 2^-24 M2) = {ratio:.3g}")
        assert (err <= bound).all(), (name, ratio)


def test_geometry_grad_is_the_two_calls(ctx):
    case = S.CASES[0]
    c, r, s, o, sh = S.scene()
    G = reference(case, True)[0]
    ubo = TG.camera(case)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        seen = {}
        frame = sc.splat_grad

        def recorded(*a, **k):  # the rows geometry_grad's own frame produced (float atomics: another frame's bits may differ)
            seen["rows"] = frame(*a, **k)
            return seen["rows"]

        sc.splat_grad = recorded
        gc, gv, go = sc.geometry_grad(ubo, G)
        del sc.splat_grad
        gc2, gv2 = sc.model_grad(ubo, seen["rows"])
    finally:
        sc.close()
    assert gc.tobytes() == gc2.tobytes() and gv.tobytes() == gv2.tobytes() and go.tobytes() == seen["rows"][:, 5].tobytes()
    assert gc.any() and gv.any() and go.any()


def test_accumulate_adds_frames(ctx):
    """as test_opacity_grad_gpu.py tests its table: a frame that writes over sentinels, a second one of another camera that
    adds; held to the sum of the two float64 references with the sum of their bounds. The projection's backward: twice
    the same rows is twice the table, exactly."""
    import torch

    cases = [S.CASES[0], S.CASES[3]]  # origin and moved, 48x32, 4 spp
    c, r, s, o, sh = S.scene()
    refs = [reference(case, True) for case in cases]
    cams = [TG.camera(case) for case in cases]
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        d_t = torch.full((S.N, 8), 123.0, dtype=torch.float32, device="cuda:0")
        d_g = [torch.from_numpy(np.ascontiguousarray(ref[0])).to("cuda:0") for ref in refs]
        sc.splat_grad_async(cams[0], d_g[0].data_ptr(), d_t.data_ptr(), accumulate=False)  # overwrites the sentinels
        sc.splat_grad_async(cams[1], d_g[1].data_ptr(), d_t.data_ptr(), accumulate=True)
        ctx.synchronize()
        got = d_t.cpu().numpy()
        out = np.zeros((S.N, 8), np.float32)  # a host table cannot accumulate
        st = gsrt.lib.gsrt_render_splat_grad(sc.handle, gsrt._p(cams[0]), gsrt.MODE_COR, 0, gsrt._p(refs[0][0]), gsrt._p(out), 1)
        assert st == gsrt.E_ARG and "SPLAT_GRAD" in gsrt.lib.gsrt_last_error(ctx.handle).decode()
        # the chain kernel
        d_c = torch.full((S.N, 3), 5.0, dtype=torch.float32, device="cuda:0")
        d_v = torch.full((S.N, 6), -5.0, dtype=torch.float32, device="cuda:0")
        sc.model_grad_async(cams[1], d_t.data_ptr(), d_c.data_ptr(), d_v.data_ptr(), accumulate=False)
        ctx.synchronize()
        once = d_c.cpu().numpy(), d_v.cpu().numpy()
        sc.model_grad_async(cams[1], d_t.data_ptr(), d_c.data_ptr(), d_v.data_ptr(), accumulate=True)
        ctx.synchronize()
        twice = d_c.cpu().numpy(), d_v.cpu().numpy()
    finally:
        sc.close()
    assert not u32(got[:, 6:]).any()
    ref = refs[0][1].rows + refs[1][1].rows
    M = refs[0][1].M + refs[1][1].M
    err = np.abs(got.astype(np.float64) - ref)[:, :6]
    reached = M[:, :6] > 0
    print(f"splat-grad accumulate: worst error / (1e-3 M) = {(err[reached] / (TG.TOL * M[:, :6][reached])).max():.3g}")
    assert (err <= TG.TOL * M[:, :6]).all() and not u32(got[:, :6])[~reached].any()
    assert np.abs(refs[1][1].rows).max() > 0
    for a, b in zip(once, twice):
        assert a.any() and (2.0 * a).tobytes() == b.tobytes()


def test_render_model_backward(ctx):
    """center.grad against Scene.geometry_grad's centres of the same scene and upstream gradient: two splat gradient
    frames (float atomics, and cov3d formed by torch here and by the library's scene build there), each within 1e-3 M of
    the float64 rows where test_rows_* hold, so their centres differ by at most the chain's absolute products of 2e-3 M,
    plus twice the chain kernel's own rounding bound (test_chain_kernel_matches_f64; kappa <= 1.7 here) and as much again
    for the two builds' float32 parameters, which differ in their last bits. rot.grad and scale.grad are
    finite and of the right shapes; the scene the forward leaves renders as one built from the same tensors."""
    import torch

    from gsrt.autograd import render_model

    case = S.CASES[0]
    c, r, s, o, sh = S.scene()
    G, sg, want = reference(case, True)
    ubo = TG.camera(case)
    d_G = torch.from_numpy(np.ascontiguousarray(G)).to("cuda:0")
    t = {k: torch.from_numpy(a).to("cuda:0").requires_grad_(True) for k, a in dict(c=c, r=r, s=s, o=o, sh=sh).items()}
    fresh = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    # the scene render_model drives: built from other values, so that what it renders is what the forward put there
    sc = gsrt.Scene.from_model(ctx, c + np.float32(0.05), r, s * np.float32(1.1), o * np.float32(0.5), sh)
    try:
        fresh.build_bvh()
        sc.build_bvh()
        plain = fresh.render(ubo)[0]
        gc = fresh.geometry_grad(ubo, G)[0]
        rgba = render_model(sc, ubo, t["c"], t["r"], t["s"], t["o"], t["sh"])
        (rgba * d_G).sum().backward()
        after = sc.render(ubo)[0]
        fwd = rgba.detach().cpu().numpy()
    finally:
        sc.close()
        fresh.close()
    assert np.abs(after - plain).max() <= 1e-3 and np.abs(fwd - plain).max() <= 1e-3
    assert np.abs(fwd.astype(np.float64) - want).max() <= 1e-3
    grads = {k: v.grad.cpu().numpy() for k, v in t.items()}
    assert grads["c"].shape == (S.N, 3) and grads["r"].shape == (S.N, 4) and grads["s"].shape == (S.N, 3)
    assert grads["o"].shape == (S.N,) and grads["sh"].shape == (S.N, 16, 3)
    assert all(np.isfinite(g).all() and g.any() for g in grads.values())
    c64, cov = c.astype(np.float64), Q.cov6(F.covariance(r, s))
    M2 = Q.model_chain(ubo, c64, cov, sg.M).M2_center
    err = np.abs(grads["c"].astype(np.float64) - gc)
    reached = M2 > 0
    tol = 2 * TG.TOL + 4 * CHAIN_OPS * (1 + 1.7) * EPS  # 2e-3 + 2.4e-5
    print(f"render_model centre gradient against geometry_grad: worst difference / ({tol:.4g} M2) = "
          f"{(err[reached] / (tol * M2[reached])).max():.3g}")
    assert (err <= tol * M2).all()
    # slot 5 came back as the opacity gradient
    TG.hold("render_model opacity", case, sg.near, grads["o"], sg.rows[:, 5], sg.M[:, 5])
