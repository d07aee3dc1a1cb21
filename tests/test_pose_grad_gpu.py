"""The camera's gradient on the GPU (gsrt_pose_grad, Scene.pose_grad, gsrt.autograd.render_model(view=...)) against the float64
one of tests/cor_f64_pose.py, which tests/test_pose_ref.py checks on the CPU, on the cases of tests/pose_cases.py.

Bound, per entry of the 4x4: |got - ref| <= sum_g N (1 + kappa_g) 2^-24 Mg + 2^-24 |ref|, ref = pose_chain of the same float32
rows and the scene's own float32 parameters (Scene.download), Mg the chain on absolute values per Gaussian, kappa_g = v00 v11 /
det as tests/test_geom_grad_gpu.py uses it, N the longest chain of rounded operations in the kernel as written (its header
counts them: 35, depth form 36; asserted below against the chain kernel's 37 and 38). N is counted, never tuned: a worst
ratio above 1 means the kernel or the count is wrong. tests/test_pose_ref.py shows that the bound sees a dropped direct term,
a transposed result, an ignored slot 6 and a dropped bottom row at least ten times over on these cases.
Measured ratios: DESIGN.md and profiles/pose_grad/.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import cor_f64_pose as PQ
import gsrt
import oracle as O
import pose_cases as PC
import test_depth_grad_f64 as SD
import test_depth_grad_gpu as TD
import test_geom_grad_gpu as TQ
import test_grad_f64 as S
import test_grad_f64_gpu as TG
from test_features_gpu import u32

pytestmark = pytest.mark.gpu

REAL_CASES = [S.CASES[0], S.CASES[3], S.CASES[-1]]


def test_counts_and_layout():
    """N is the chain kernel's count less its final MV^T dL/dt (4) plus the outer product and the direct term's sum (2);
    the seams are placed by what the library reports"""
    assert PC.N_OPS == {False: TQ.CHAIN_OPS - 4 + 2, True: TD.CHAIN_OPS - 4 + 2} == {False: 35, True: 36}
    assert gsrt.pose_grad_layout() == (PC.CHUNK, PC.LANES)
    assert [n for n, _ in PC.seam_sizes()][-1] == PC.LANES * PC.CHUNK + 1


def hold(label, case, got, G, B):
    """every entry within the bound; entries nothing reaches are +0; the worst ratio printed in test_grad_f64_gpu.hold's
    line format and appended to COR_F64_REPORT"""
    got = np.asarray(got)
    assert got.shape == (16,) and got.dtype == np.float32 and np.isfinite(got).all()
    g = PQ.mat(got)
    err = np.abs(g - G)
    reached = B > 0
    worst = float((err[reached] / B[reached]).max())
    print(f"{label} {case}: {reached.sum()} of 16 entries reached; worst error / (sum N (1 + kappa) 2^-24 Mg + 2^-24 |ref|) "
          f"= {worst:.3g}")
    rep = os.environ.get("COR_F64_REPORT")
    if rep:
        with open(rep, "a") as fh:
            fh.write(json.dumps({"case": f"{label} {case}", "entries": 16, "worst_ratio": worst}) + "\n")
    assert not u32(got)[~reached.T.reshape(16)].any(), label  # got[c * 4 + r] is entry [r, c]
    assert (err <= B).all(), f"{label}: worst error / bound = {worst:.3g}"
    assert reached.sum() >= 12
    return worst


def built(ctx, params, aabbs):
    sc = gsrt.Scene.from_params(ctx, params, aabbs)
    sc.build_bvh()
    return sc


@pytest.mark.parametrize("n,depth", PC.seam_cases(), ids=lambda v: str(v))
def test_seams_match_f64(ctx, n, depth):
    """synthetic rows and parameters at the sizes where the kernels take another path. A sixth of the Gaussians stand
    behind the camera with rows of ones and contribute nothing: a second run with their rows zeroed gives the same bits."""
    ubo = PC.camera()
    params, aabbs, rows, behind = PC.synthetic(n, 100 + n % 97)
    sc = built(ctx, params, aabbs)
    try:
        down, _ = sc.download()
        got = sc.pose_grad(ubo, rows, depth=depth)
        zeroed = rows.copy()
        zeroed[behind] = 0.0
        again = sc.pose_grad(ubo, zeroed, depth=depth)
    finally:
        sc.close()
    assert down.tobytes() == params.tobytes()
    G, B, valid = PC.reference(ubo, down, rows, depth)
    assert not valid[behind].any() and valid.sum() == n - behind.sum()
    assert got.tobytes() == again.tobytes()
    hold("pose-grad seam depth" if depth else "pose-grad seam", n, got, G, B)


@pytest.mark.parametrize("case", REAL_CASES, ids=lambda c: "%s-%dx%d-spp%d" % c)
def test_real_rows_match_f64(ctx, case):
    """the rows of Scene.splat_grad and Scene.splat_depth_grad of three of test_geom_grad_gpu's frames"""
    c, r, s, o, sh = S.scene()
    ubo = TG.camera(case)
    G = S.upstream(case, 4, 201 + case[3], True)
    Gd = SD.upstream_depth(case, 301 + case[3], True)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        down, _ = sc.download()
        plain = sc.splat_grad(ubo, G)
        deep = sc.splat_depth_grad(ubo, G, Gd)
        got = sc.pose_grad(ubo, plain), sc.pose_grad(ubo, deep, depth=True)
    finally:
        sc.close()
    assert plain.any() and deep[:, 6].any()
    for depth, rows, g in ((False, plain, got[0]), (True, deep, got[1])):
        Gref, B, _ = PC.reference(ubo, down, rows, depth)
        hold("pose-grad real rows depth" if depth else "pose-grad real rows", case, g, Gref, B)
    assert got[0].tobytes() != got[1].tobytes()


@pytest.mark.parametrize("depth", [False, True], ids=["plain", "depth"])
def test_nonaffine_view_and_general_projection(ctx, depth):
    """a model-view whose bottom row is not (0, 0, 0, 1) and a projection with every entry the kernel reads non-zero: the
    bottom row of the gradient is reached"""
    ubo = PC.nonaffine_camera()
    params, aabbs, rows, _ = PC.synthetic(777, 21, ubo)
    sc = built(ctx, params, aabbs)
    try:
        got = sc.pose_grad(ubo, rows, depth=depth)
    finally:
        sc.close()
    G, B, valid = PC.reference(ubo, params, rows, depth)
    assert valid.sum() > 500 and (B > 0).all() and np.abs(G[3]).min() > 0
    hold("pose-grad non-affine depth" if depth else "pose-grad non-affine", 777, got, G, B)


@pytest.mark.parametrize("depth", [False, True], ids=["plain", "depth"])
def test_translation_column_is_the_centre_gradient_bit_for_bit(ctx, depth):
    """gsrt_pose_grad and gsrt_splat_grad_to_model carry one dL/dt (cor_chain_grad): for a single Gaussian under a view
    whose 3x3 is the identity, the gradient's translation column equals the centre's gradient exactly. Column 3 of the pose
    contribution is gt[r] * 1 with no direct term, and the double sum of one term rounds back to the same float; the centre's
    MV^T gt is ((1 gt[k] + 0) + 0) + 0 gt[3]. Compared as floats (a zero's sign would not matter), and every value
    non-zero: 16 seeded Gaussians with random rows under a general projection."""
    P = PC.nonaffine_camera()["projection"][0]
    rng = np.random.default_rng(1601)
    for seed in range(16):
        mv = O.translate(*rng.uniform(-2.0, 2.0, 3))
        ubo = PC.camera(mv, P)
        assert ubo["model_view"][0].tobytes() == mv.tobytes() and (ubo["projection"][0] != 0).sum() >= 12
        params, aabbs, rows, behind = PC.synthetic(1, 500 + seed, ubo)
        assert not behind.any() and rows[0, :7].all()
        sc = built(ctx, params, aabbs)
        try:
            pose = sc.pose_grad(ubo, rows, depth=depth)
            centre, _ = sc.model_grad(ubo, rows, depth=depth)
        finally:
            sc.close()
        assert pose[12:15].all() and (pose[12:15] == centre[0]).all(), (seed, pose[12:16], centre[0])


def test_deterministic_across_calls_and_workspace_regrowth():
    """two calls give equal bits, and so does a call after a larger one has regrown the context's workspace (a context of
    its own, so that the workspace starts small)"""
    ubo = PC.camera()
    small = PC.synthetic(3 * PC.CHUNK + 17, 7)
    large = PC.synthetic(40 * PC.CHUNK + 5, 8)
    with gsrt.Context(0) as own:
        a, b = built(own, small[0], small[1]), built(own, large[0], large[1])
        try:
            first = a.pose_grad(ubo, small[2])
            second = a.pose_grad(ubo, small[2])
            big = b.pose_grad(ubo, large[2])
            third = a.pose_grad(ubo, small[2])
            big2 = b.pose_grad(ubo, large[2])
        finally:
            a.close()
            b.close()
    assert first.any() and first.tobytes() == second.tobytes() == third.tobytes()
    assert big.tobytes() == big2.tobytes() and big.tobytes() != first.tobytes()


def test_async_and_device_rows_equal_blocking(ctx):
    import torch

    ubo = PC.camera()
    params, aabbs, rows, _ = PC.synthetic(PC.CHUNK + 1, 13)
    sc = built(ctx, params, aabbs)
    try:
        d_rows = torch.from_numpy(rows).to("cuda:0")
        torch.cuda.synchronize()
        for depth in (False, True):
            host = sc.pose_grad(ubo, rows, depth=depth)
            dev = sc.pose_grad(ubo, d_rows.data_ptr(), depth=depth)
            d_out = torch.full((16,), 9.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            sc.pose_grad_async(ubo, d_rows.data_ptr(), d_out.data_ptr(), depth=depth)
            ctx.synchronize()
            assert host.any() and host.tobytes() == dev.tobytes() == d_out.cpu().numpy().tobytes()
    finally:
        sc.close()


def test_refusals_leave_the_output_untouched(ctx):
    import torch

    L, p, P = gsrt.lib, gsrt._p, ctypes.c_void_p
    ubo = PC.camera()
    params, aabbs, rows, _ = PC.synthetic(100, 3)
    out = np.full(16, 5.0, np.float32)
    d_out = torch.full((16,), 5.0, dtype=torch.float32, device="cuda:0")
    d_rows = torch.from_numpy(rows).to("cuda:0")
    torch.cuda.synchronize()

    def last():
        return L.gsrt_last_error(ctx.handle).decode()

    sc = gsrt.Scene.from_params(ctx, params, aabbs)
    try:
        assert L.gsrt_pose_grad(sc.handle, p(ubo), p(rows), 0, p(out)) == gsrt.E_STATE and "gsrt_build_bvh" in last()
        assert L.gsrt_pose_grad_async(sc.handle, p(ubo), P(d_rows.data_ptr()), 0, P(d_out.data_ptr())) == gsrt.E_STATE
        sc.build_bvh()
        assert L.gsrt_pose_grad(sc.handle, p(ubo), None, 0, p(out)) == gsrt.E_ARG and "grad_splat is NULL" in last()
        assert L.gsrt_pose_grad(sc.handle, p(ubo), p(rows), 1, None) == gsrt.E_ARG and "grad_model_view is NULL" in last()
        assert L.gsrt_pose_grad(sc.handle, None, p(rows), 0, p(out)) == gsrt.E_ARG
        assert L.gsrt_pose_grad_async(sc.handle, p(ubo), None, 0, P(d_out.data_ptr())) == gsrt.E_ARG
        assert L.gsrt_pose_grad_async(sc.handle, p(ubo), P(d_rows.data_ptr()), 0, None) == gsrt.E_ARG
        v, i = gsrt.sphere_mesh((0.0, 0.0, -4.0), 0.5)
        sc.add_mesh(v, i)
        assert L.gsrt_pose_grad(sc.handle, p(ubo), p(rows), 0, p(out)) == gsrt.E_ARG and "mesh" in last()
        assert L.gsrt_pose_grad_async(sc.handle, p(ubo), P(d_rows.data_ptr()), 0, P(d_out.data_ptr())) == gsrt.E_ARG
    finally:
        sc.close()
    ctx.synchronize()
    assert (out == 5.0).all() and (d_out.cpu().numpy() == 5.0).all()


def _tensors(arrays):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0").requires_grad_(True) for a in arrays]


def test_render_model_view(ctx):
    """render_model(view=V): the frame is view=None's bit for bit (for a ubo that holds V and its float64 inverse); V.grad
    is Scene.pose_grad of rows recomputed from the same upstream gradient, within the sum of both bounds plus the rows'
    own difference (float atomics reorder: two frames' rows differ by at most 2 TOL M, tests/test_geom_grad_gpu.py); with
    depth=True a loss on the depth alone gives a non-zero gradient."""
    import torch

    from gsrt.autograd import render_model

    case = S.CASES[0]
    c, r, s, o, sh = S.scene()
    ubo = TG.camera(case)
    G = S.upstream(case, 4, 201 + case[3], True)
    Gd = SD.upstream_depth(case, 301 + case[3], True)
    mv = ubo["model_view"][0]
    held = ubo.copy()
    inv = torch.linalg.inv(torch.from_numpy(PQ.mat(mv)))  # as the forward forms it: float64, rounded once
    held["model_view_inverse"][0] = inv.t().contiguous().reshape(16).to(torch.float32).numpy()
    V = torch.from_numpy(np.ascontiguousarray(mv.reshape(4, 4).T)).to("cuda:0").requires_grad_(True)
    d_G = torch.from_numpy(np.ascontiguousarray(G)).to("cuda:0")
    d_Gd = torch.from_numpy(np.ascontiguousarray(Gd)).to("cuda:0")
    t = _tensors((c, r, s, o, sh))
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        with torch.no_grad():
            plain = render_model(sc, held, *t).cpu().numpy()
        rgba = render_model(sc, ubo, *t, view=V)
        assert rgba.detach().cpu().numpy().tobytes() == plain.tobytes()
        (rgba * d_G).sum().backward()
        got = V.grad.cpu().numpy().copy()
        centre_grad = t[0].grad.cpu().numpy().copy()
        down, _ = sc.download()
        rows = sc.splat_grad(held, G)
        want = sc.pose_grad(held, rows)
        # the depth path
        V.grad = None
        rgba2, dep = render_model(sc, ubo, *t, depth=True, view=V)
        (dep * d_Gd).sum().backward()
        deep = V.grad.cpu().numpy().copy()
        rows_d = sc.splat_depth_grad(held, np.zeros_like(G), Gd)
        want_d = sc.pose_grad(held, rows_d, depth=True)
        # view=None leaves the other gradients as they were
        for x in t:
            x.grad = None
        (render_model(sc, held, *t) * d_G).sum().backward()
        centre_plain = t[0].grad.cpu().numpy()
    finally:
        sc.close()
    assert got.shape == (4, 4) and got.dtype == np.float32 and np.isfinite(got).all() and got.any()
    assert deep.shape == (4, 4) and np.isfinite(deep).all() and deep[:3].any()
    # the float64 magnitudes of the two frames' rows: each frame's rows are within TOL M of the float64 rows
    # (tests/test_geom_grad_gpu.py, tests/test_depth_grad_gpu.py), so two frames differ by at most 2 TOL M, chained
    import cor_f64_depth as D

    M_plain = TQ.reference(case, True)[1].M
    M_deep = D.depth_gradients(held, c, r, s, o, sh, G_rgba=np.zeros_like(G, np.float64), G_depth=Gd).M
    p64 = down.astype(np.float64)
    for label, g44, w16, rws, Mrows, depth in (("colour", got, want, rows, M_plain, False),
                                               ("depth", deep, want_d, rows_d, M_deep, True)):
        _, B, _ = PC.reference(held, down, rws, depth)
        M = PQ.pose_chain(held, p64[:, :3], p64[:, 4:10], Mrows, depth).M
        tol = 2 * B + 2 * TG.TOL * M
        err = np.abs(g44.astype(np.float64) - PQ.mat(w16))
        print(f"render_model view gradient ({label}) against Scene.pose_grad: worst difference / tolerance = "
              f"{(err[tol > 0] / tol[tol > 0]).max():.3g}")
        assert (err <= tol).all()
    assert np.abs(centre_grad.astype(np.float64) - centre_plain).max() <= 1e-2 * np.abs(centre_plain).max()


def test_refinement_recovers_a_perturbed_pose(ctx):
    """Tracking against a fixed map: an SH-less scene of 300 Gaussians at 64x64, the target rendered at pose P*; from
    exp(xi0^) P*, xi0 a rotation of a fraction of a pixel plus a translation, 30 steps of Adam in twist space with
    photometric_loss, pose_twist and ubo_apply_twist. The final loss is below the initial loss and the final pose error
    |log(P P*^-1)| below the initial one; no rate is fixed. The end points go to POSE_REFINE_REPORT when it is set."""
    import torch

    from gsrt.autograd import photometric_loss

    c, r, s, o, _ = S.scene()
    n = len(c)
    star = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, 64, 64, 1.0, 1, 16)
    pixel = 2.0 * np.tan(np.radians(30.0)) / 64.0  # the angle one pixel subtends
    xi0 = np.array([0.004, -0.003, 0.002, 0.3 * pixel, -0.4 * pixel, 0.2 * pixel], np.float32)
    ubo = gsrt.ubo_apply_twist(star, xi0)
    Pstar = PQ.mat(star["model_view"][0])

    def pose_error(u):
        return float(np.linalg.norm(PQ.log_twist(PQ.mat(u["model_view"][0]) @ np.linalg.inv(Pstar))))

    sc = gsrt.Scene.from_model(ctx, c, r, s, o)
    losses, errors = [], [pose_error(ubo)]
    try:
        sc.build_bvh()
        target = torch.from_numpy(sc.render(star)[0]).to("cuda:0")
        rgba = torch.empty((64, 64, 4), dtype=torch.float32, device="cuda:0")
        rows = torch.empty((n, 8), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        m, v = np.zeros(6), np.zeros(6)
        # rates set beforehand from the geometry, not from a run: a rotation step of pixel / 90 lets 30 steps cover a third
        # of a pixel, the size of the perturbation; the translation, which at this scene's depths moves the image far
        # less than the rotation does, steps a tenth of that, so that it cannot absorb the rotation's image shift
        lr = np.array([pixel / 900.0] * 3 + [pixel / 90.0] * 3)
        b1, b2 = 0.9, 0.999
        for step in range(1, 32):
            sc.render_async(ubo, d_rgba=rgba.data_ptr())
            ctx.synchronize()
            x = rgba.clone().requires_grad_(True)
            loss = photometric_loss(ctx, x, target, lam=0.2)
            loss.backward()
            losses.append(float(loss.detach()))
            if step == 31:
                break
            gimg = x.grad.contiguous()
            torch.cuda.synchronize()
            sc.splat_grad_async(ubo, gimg.data_ptr(), rows.data_ptr())
            g = gsrt.pose_twist(ubo["model_view"][0], sc.pose_grad(ubo, rows.data_ptr())).astype(np.float64)
            m, v = b1 * m + (1 - b1) * g, b2 * v + (1 - b2) * g * g
            upd = -lr * (m / (1 - b1 ** step)) / (np.sqrt(v / (1 - b2 ** step)) + 1e-12)
            ubo = gsrt.ubo_apply_twist(ubo, upd.astype(np.float32))
            errors.append(pose_error(ubo))
    finally:
        sc.close()
    print(f"pose refinement: loss {losses[0]:.6g} -> {losses[-1]:.6g}, pose error {errors[0]:.6g} -> {errors[-1]:.6g} "
          f"after {len(errors) - 1} steps")
    rep = os.environ.get("POSE_REFINE_REPORT")
    if rep:
        with open(rep, "a") as fh:
            fh.write(json.dumps({"steps": len(errors) - 1, "loss": [losses[0], losses[-1]],
                                 "pose_error": [errors[0], errors[-1]]}) + "\n")
    assert losses[-1] < losses[0] and errors[-1] < errors[0]
