"""The depth backward on the GPU against the float64 one of tests/cor_f64_depth.py (checked on the CPU by
tests/test_depth_grad_f64.py): the splat-depth gradient frame (gsrt_render_splat_depth_grad), the depth chain
(gsrt_splat_depth_grad_to_model), Scene.geometry_grad(grad_depth=...), accumulate, and
gsrt.autograd.render_model(depth=True).

Scene, cameras, upstream gradients and frames are those of tests/test_grad_f64_gpu.py (300 Gaussians, frames of at most
48x32 pixels, 1, 3 and 4 spp); its reference cache, `hold` (every entry within 1e-3 M, entries nothing reaches +0, the worst
ratio printed and appended to COR_F64_REPORT) and frame_checks are used as they are. G and Gdepth (seeded normal noise) are
zero on the float32-sensitive pixels. Measured ratios: DESIGN.md section 5.
"""
import numpy as np
import pytest

import cor_f64 as F
import cor_f64_depth as D
import cor_f64_geom as Q
import gsrt
import test_depth_grad_f64 as SD
import test_geom_grad_gpu as TQ
import test_grad_f64 as S
import test_grad_f64_gpu as TG
from test_features_gpu import u32

pytestmark = pytest.mark.gpu

CASES = TG.CASES
# k_splat_grad_to_model<true> as it is written: the parent's 37 (tests/test_geom_grad_gpu.py lists them) and one more rounded
# operation on the longest chain, dL/dt2 - row[6], between the ppx, ppy part and MV^T dL/dt
CHAIN_OPS = TQ.CHAIN_OPS + 1
EPS = TQ.EPS
_REF = {}


def reference(case, with_sh):
    """TG.reference's G and frame, Gdepth, and the float64 splat-depth rows of both; computed once per case"""
    key = (case, with_sh)
    if key not in _REF:
        c, r, s, o, sh = S.scene()
        G, ref, want = TG.reference(case, with_sh)
        Gd = SD.upstream_depth(case, 301 + case[3], with_sh)
        dg = D.depth_gradients(TG.camera(case), c, r, s, o, sh if with_sh else None, G_rgba=G, G_depth=Gd)
        assert dg.digest == ref.digest and np.array_equal(dg.near, ref.near)
        _REF[key] = (G, Gd, dg, want)
    return _REF[key]


def rows_check(label, ctx, case, with_sh):
    c, r, s, o, sh = S.scene()
    G, Gd, dg, want = reference(case, with_sh)
    ubo = TG.camera(case)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh if with_sh else None)
    try:
        sc.build_bvh()
        got = sc.splat_depth_grad(ubo, G, Gd)
        TG.frame_checks(ctx, sc, ubo, case, want)
    finally:
        sc.close()
    assert got.shape == (S.N, 8) and got.dtype == np.float32
    assert not u32(got[:, 7]).any()  # slot 7: all bits zero
    TG.hold(label, case, dg.near, got[:, :7], dg.rows[:, :7], dg.M[:, :7])


@CASES
def test_rows_with_sh_match_f64(ctx, case):
    rows_check("splat-depth-grad SH", ctx, case, True)


@CASES
def test_rows_without_sh_match_f64(ctx, case):
    rows_check("splat-depth-grad colour 1", ctx, case, False)


@pytest.mark.parametrize("case", [S.CASES[0], S.CASES[4]], ids=lambda c: "%s-%dx%d-spp%d" % c)
def test_zero_depth_gradient_is_the_splat_frame(ctx, case):
    """Gdepth = 0: slots 0..5 held to cor_f64_geom.splat_gradients of the same G, slot 6 all bits zero"""
    c, r, s, o, sh = S.scene()
    G, sg, _ = TQ.reference(case, True)
    ubo = TG.camera(case)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        got = sc.splat_depth_grad(ubo, G, np.zeros(G.shape[:2], np.float32))
    finally:
        sc.close()
    assert not u32(got[:, 6:]).any()
    TG.hold("splat-depth-grad Gdepth 0", case, sg.near, got[:, :6], sg.rows[:, :6], sg.M[:, :6])


@pytest.mark.parametrize("case", [S.CASES[0], S.CASES[5]], ids=lambda c: "%s-%dx%d-spp%d" % c)
def test_unit_depth_gradient_is_the_blend_weight(ctx, case):
    """G = 0, Gdepth = 1: slot 6 held to the float64 summed blend weight per Gaussian (over ns). No Gaussian of this scene
    is only ever clamped (a splat clamped near its centre is open at its rim, tests/test_depth_grad_f64.py), so the hits
    the clamp replaced are reached through the Gaussians that take more than 40 TOL of their weight through them: a slot 6
    that left clamped hits out would miss the bound on those forty times over."""
    c, r, s, o, sh = S.scene()
    _, w, h, _ = case
    ubo = TG.camera(case)
    ones = D.depth_gradients(ubo, c, r, s, o, sh, G_rgba=np.zeros((h, w, 4)), G_depth=np.ones((h, w)))
    assert (ones.weight_clamped > 40 * TG.TOL * ones.weight).any()
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        got = sc.splat_depth_grad(ubo, np.zeros((h, w, 4), np.float32), np.ones((h, w), np.float32))
    finally:
        sc.close()
    assert not u32(got[:, 7]).any()
    TG.hold("splat-depth-grad weight", case, ones.near, got[:, 6], ones.weight, ones.weight)
    heavy = ones.weight_clamped > 40 * TG.TOL * ones.weight
    assert (got[heavy, 6] > 0).all()
    assert (np.abs(got[heavy, 6] - ones.weight[heavy]) < 0.5 * ones.weight_clamped[heavy]).all()
    # slots 0..5 of this frame are the depth's own backward: held too
    TG.hold("splat-depth-grad depth alone", case, ones.near, got[:, :6], ones.rows[:, :6], ones.M[:, :6])


@pytest.mark.parametrize("case", [S.CASES[0], S.CASES[3], S.CASES[-1]], ids=lambda c: "%s-%dx%d-spp%d" % c)
def test_chain_kernel_matches_f64(ctx, case):
    """Scene.model_grad(depth=True) of the float32 reference rows against depth_chain of those same rows and the scene's own
    float32 parameters, as tests/test_geom_grad_gpu.py holds the plain chain: per entry |got - ref| <= CHAIN_OPS (1 +
    kappa_g) 2^-24 M2 with CHAIN_OPS = 38. Six Gaussians are moved behind the camera and given rows of ones: invalid splats
    get +0. grad_cov is the plain chain's on the same rows, byte for byte."""
    c, r, s, o, _ = S.scene()
    dg = reference(case, True)[2]
    ubo = TG.camera(case)
    behind = np.arange(0, S.N, S.N // 6)[:6]
    c = c.copy()
    mv = F.Ubo(ubo).MV
    c[behind] = (np.linalg.inv(mv) @ np.array([0.3, -0.2, 2.5, 1.0]))[:3].astype(np.float32)  # view z > 0: depth < 0
    rows = dg.rows.astype(np.float32)
    rows[behind] = 1.0
    sc = gsrt.Scene.from_model(ctx, c, r, s, o)
    try:
        sc.build_bvh()
        params, _ = sc.download()
        gc, gv = sc.model_grad(ubo, rows, depth=True)
        gc0, gv0 = sc.model_grad(ubo, rows)
    finally:
        sc.close()
    ref = D.depth_chain(ubo, params[:, :3].astype(np.float64), params[:, 4:10].astype(np.float64), rows.astype(np.float64))
    assert not ref.valid[behind].any() and ref.valid.sum() == S.N - 6
    assert gc.shape == (S.N, 3) and gv.shape == (S.N, 6) and np.isfinite(gc).all() and np.isfinite(gv).all()
    assert not u32(gc[behind]).any() and not u32(gv[behind]).any()
    assert gv.tobytes() == gv0.tobytes() and gc.tobytes() != gc0.tobytes()
    for name, got, want, M2 in (("centre", gc, ref.center, ref.M2_center), ("cov", gv, ref.cov, ref.M2_cov)):
        bound = CHAIN_OPS * (1.0 + ref.kappa[:, None]) * EPS * M2
        err = np.abs(got.astype(np.float64) - want)
        reached = M2 > 0
        assert reached.sum() > M2.size // 4
        ratio = float((err[reached] / bound[reached]).max())
        print(f"depth model-grad {name} {case}: worst error / (N (1 + kappa) 2^-24 M2) = {ratio:.3g}")
        assert (err <= bound).all(), (name, ratio)


def test_geometry_grad_is_the_two_calls(ctx):
    case = S.CASES[0]
    c, r, s, o, sh = S.scene()
    G, Gd = reference(case, True)[:2]
    ubo = TG.camera(case)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        seen = {}
        frame, plain = sc.splat_depth_grad, sc.splat_grad

        def recorded(*a, **k):  # the rows geometry_grad's own frame produced (float atomics: another frame's bits may differ)
            seen["rows"] = frame(*a, **k)
            return seen["rows"]

        def recorded_plain(*a, **k):
            seen["plain"] = plain(*a, **k)
            return seen["plain"]

        sc.splat_depth_grad, sc.splat_grad = recorded, recorded_plain
        gc, gv, go = sc.geometry_grad(ubo, G, grad_depth=Gd)
        assert "plain" not in seen
        pc, pv, po = sc.geometry_grad(ubo, G)  # grad_depth=None: today's two calls
        del sc.splat_depth_grad, sc.splat_grad
        gc2, gv2 = sc.model_grad(ubo, seen["rows"], depth=True)
        pc2, pv2 = sc.model_grad(ubo, seen["plain"])
    finally:
        sc.close()
    assert gc.tobytes() == gc2.tobytes() and gv.tobytes() == gv2.tobytes() and go.tobytes() == seen["rows"][:, 5].tobytes()
    assert pc.tobytes() == pc2.tobytes() and pv.tobytes() == pv2.tobytes() and po.tobytes() == seen["plain"][:, 5].tobytes()
    assert gc.any() and gv.any() and go.any() and seen["rows"][:, 6].any() and not seen["plain"][:, 6].any()


def test_accumulate_adds_frames(ctx):
    """as tests/test_geom_grad_gpu.py tests its table: a frame that writes over sentinels, a second one of another camera
    that adds; held to the sum of the two float64 references with the sum of their bounds. The depth chain: twice the same
    rows is twice the table, exactly."""
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
        d_gd = [torch.from_numpy(np.ascontiguousarray(ref[1])).to("cuda:0") for ref in refs]
        sc.splat_depth_grad_async(cams[0], d_g[0].data_ptr(), d_gd[0].data_ptr(), d_t.data_ptr(), accumulate=False)
        sc.splat_depth_grad_async(cams[1], d_g[1].data_ptr(), d_gd[1].data_ptr(), d_t.data_ptr(), accumulate=True)
        ctx.synchronize()
        got = d_t.cpu().numpy()
        out = np.zeros((S.N, 8), np.float32)  # a host table cannot accumulate
        st = gsrt.lib.gsrt_render_splat_depth_grad(sc.handle, gsrt._p(cams[0]), gsrt.MODE_COR, 0, gsrt._p(refs[0][0]),
                                                   gsrt._p(refs[0][1]), gsrt._p(out), 1)
        assert st == gsrt.E_ARG and "GSRT_FLAG_SPLAT_DEPTH_GRAD" in gsrt.lib.gsrt_last_error(ctx.handle).decode()
        d_c = torch.full((S.N, 3), 5.0, dtype=torch.float32, device="cuda:0")
        d_v = torch.full((S.N, 6), -5.0, dtype=torch.float32, device="cuda:0")
        sc.model_grad_async(cams[1], d_t.data_ptr(), d_c.data_ptr(), d_v.data_ptr(), accumulate=False, depth=True)
        ctx.synchronize()
        once = d_c.cpu().numpy(), d_v.cpu().numpy()
        sc.model_grad_async(cams[1], d_t.data_ptr(), d_c.data_ptr(), d_v.data_ptr(), accumulate=True, depth=True)
        ctx.synchronize()
        twice = d_c.cpu().numpy(), d_v.cpu().numpy()
    finally:
        sc.close()
    # the first frame wrote over the sentinel in slot 7 too (accumulate == 0 writes the table)
    assert not u32(got[:, 7]).any()
    ref = (refs[0][2].rows + refs[1][2].rows)[:, :7]
    M = (refs[0][2].M + refs[1][2].M)[:, :7]
    err = np.abs(got.astype(np.float64)[:, :7] - ref)
    reached = M > 0
    print(f"splat-depth-grad accumulate: worst error / (1e-3 M) = {(err[reached] / (TG.TOL * M[reached])).max():.3g}")
    assert (err <= TG.TOL * M).all() and not u32(got[:, :7])[~reached].any()
    assert np.abs(refs[1][2].rows[:, 6]).max() > 0
    for a, b in zip(once, twice):
        assert a.any() and (2.0 * a).tobytes() == b.tobytes()


def test_render_model_depth_backward(ctx):
    """render_model(depth=True): the forward depth within TOL times the float64 per-pixel sum |z_i| w_i of the float64 depth,
    off the float32-sensitive pixels; center.grad against Scene.geometry_grad(grad_depth=...) under
    test_render_model_backward's tolerance with the depth chain's operation count; opacity.grad held on slot 5; a second
    backward through the depth alone."""
    import torch

    from gsrt.autograd import render_model

    case = S.CASES[0]
    c, r, s, o, sh = S.scene()
    G, Gd, dg, want = reference(case, True)
    ubo = TG.camera(case)
    d_G = torch.from_numpy(np.ascontiguousarray(G)).to("cuda:0")
    d_Gd = torch.from_numpy(np.ascontiguousarray(Gd)).to("cuda:0")
    t = {k: torch.from_numpy(a).to("cuda:0").requires_grad_(True) for k, a in dict(c=c, r=r, s=s, o=o, sh=sh).items()}
    fresh = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc = gsrt.Scene.from_model(ctx, c + np.float32(0.05), r, s * np.float32(1.1), o * np.float32(0.5), sh)
    try:
        fresh.build_bvh()
        sc.build_bvh()
        gc = fresh.geometry_grad(ubo, G, grad_depth=Gd)[0]
        rgba, depth = render_model(sc, ubo, t["c"], t["r"], t["s"], t["o"], t["sh"], depth=True)
        ((rgba * d_G).sum() + (depth * d_Gd).sum()).backward()
        grads = {k: v.grad.cpu().numpy() for k, v in t.items()}
        fwd, fwd_d = rgba.detach().cpu().numpy(), depth.detach().cpu().numpy()
        for v in t.values():
            v.grad = None
        depth2 = render_model(sc, ubo, t["c"], t["r"], t["s"], t["o"], t["sh"], depth=True)[1]
        (depth2 * d_Gd).sum().backward()
        second = {k: (None if v.grad is None else v.grad.cpu().numpy()) for k, v in t.items()}
    finally:
        sc.close()
        fresh.close()
    assert np.abs(fwd.astype(np.float64) - want).max() <= 1e-3
    off = ~dg.near
    derr = np.abs(fwd_d.astype(np.float64) - dg.depth)
    print(f"render_model depth {case}: worst error / (1e-3 sum |z| w) = "
          f"{(derr[off & (dg.depth_M > 0)] / (TG.TOL * dg.depth_M[off & (dg.depth_M > 0)])).max():.3g}")
    assert (derr[off] <= TG.TOL * dg.depth_M[off]).all() and (dg.depth_M[off] > 0).sum() > off.size // 4
    assert grads["c"].shape == (S.N, 3) and grads["r"].shape == (S.N, 4) and grads["s"].shape == (S.N, 3)
    assert grads["o"].shape == (S.N,) and grads["sh"].shape == (S.N, 16, 3)
    assert all(np.isfinite(g).all() and g.any() for g in grads.values())
    c64, cov = c.astype(np.float64), Q.cov6(F.covariance(r, s))
    M2 = D.depth_chain(ubo, c64, cov, dg.M).M2_center
    err = np.abs(grads["c"].astype(np.float64) - gc)
    reached = M2 > 0
    tol = 2 * TG.TOL + 4 * CHAIN_OPS * (1 + 1.7) * EPS
    print(f"render_model depth centre gradient against geometry_grad: worst difference / ({tol:.4g} M2) = "
          f"{(err[reached] / (tol * M2[reached])).max():.3g}")
    assert (err <= tol * M2).all()
    TG.hold("render_model depth opacity", case, dg.near, grads["o"], dg.rows[:, 5], dg.M[:, 5])
    # the depth alone: geometry and opacity get finite, non-zero gradients; the SH table gets none or zeros
    for k in ("c", "r", "s", "o"):
        assert second[k] is not None and np.isfinite(second[k]).all() and second[k].any(), k
    assert second["sh"] is None or (np.isfinite(second["sh"]).all() and not second["sh"].any())
