"""Every gradient gsrt.autograd.render_model hands torch (center, rot, scale, opacity, sh) against float64, and the torch step
underneath it, gsrt.autograd.model_covariance, against float64 and against the library's own scene build.

The kernels below render_model are held one by one elsewhere (tests/test_geom_grad_gpu.py, test_depth_grad_gpu.py,
test_grad_f64_gpu.py); here the glue is: the order and convention of the six cov3d slots on their way back from
Scene.model_grad_async into torch, which argument needs_input_grad looks at, R against R transposed, the chain torch takes
from cov3d to rot and scale (tests/cor_f64_geom.py's param_chain, checked on the CPU in tests/test_geom_grad_f64.py, whose
test_param_chain_power shows that each of these faults misses the bounds used here tenfold), and a whole training step
through gsrt.autograd.photometric_loss.

Scene, cameras, upstream gradients (zero on the float32-sensitive pixels) and float64 reference caches are those of
test_geom_grad_gpu.reference and test_depth_grad_gpu.reference: 300 Gaussians, frames of at most 48x32 pixels. The cov3d
gradient is read without touching the library: model_covariance is wrapped (monkeypatch) and the wrapper hooks its result.

model_covariance, forward. Per entry |got - ref| <= N_FWD 2^-24 M, M = sum_k s_k^2 Rabs_ki Rabs_kj the sum of the absolute
values of the entry's terms (cor_f64_geom.covariance_magnitude) and N_FWD = 7 the longest chain of rounded operations from
the float32 inputs, the same count in both builds, a product counting one more than its factors together:
  model_covariance (torch): R_ki 3 (two squares or products at once, their sum, 1 - 2 (.); the doubling is exact),
                            M = s R 4, einsum: M_ki M_kj 5, three terms 7.
  k_cov3d (the scene build): R 3, M = S R 4 (the other two products of the matrix product are with 0: exact),
                            Sigma = M^T M: the product 5, three terms 7. A contraction to an fma only removes roundings.
The backward's counts, N_TORCH (scale 14, rot 19), are listed beside the constant in tests/test_geom_grad_f64.py.

render_model. cov3d's and the centres' gradients: within model_tol() M2 of model_chain / depth_chain of the float64 rows
(test_geom_grad_f64.model_tol: 1e-3 for the one GPU frame, twice the chain kernel's bound); every slot, and +0 where
nothing reaches. scale.grad and rot.grad: within (model_tol() + N_TORCH 2^-24) M of param_chain. opacity.grad and sh.grad:
test_grad_f64_gpu.hold (1e-3 M). Each comparison prints its worst error / bound in hold's line format and appends to
COR_F64_REPORT. Measured ratios: DESIGN.md section 5.
"""
import json
import os

import numpy as np
import pytest

import cor_f64 as F
import cor_f64_depth as D
import cor_f64_geom as Q
import gsrt
import test_depth_grad_gpu as TD
import test_geom_grad_f64 as SQ
import test_geom_grad_gpu as TQ
import test_grad_f64 as S
import test_grad_f64_gpu as TG
from test_features_gpu import u32

pytestmark = pytest.mark.gpu

EPS = SQ.EPS
N_FWD = 7
MODEL_CASES = [S.CASES[0], ("origin", 48, 32, 3), ("origin", 18, 18, 4)]  # 4 spp in the wave, 3 spp as passes, ragged
CASES = pytest.mark.parametrize("case", MODEL_CASES, ids=lambda c: "%s-%dx%d-spp%d" % c)
DEPTH = pytest.mark.parametrize("depth", [False, True], ids=["plain", "depth"])


def test_constants():
    assert SQ.GPU_CHAIN_OPS == TQ.CHAIN_OPS and TD.CHAIN_OPS == TQ.CHAIN_OPS + 1 and all(c in S.CASES for c in MODEL_CASES)


def hold(label, case, near, got, ref, M, tol, plus_zero=True, most=True):
    """test_grad_f64_gpu.hold with the bound tol M: every entry within it, the worst ratio printed and reported; plus_zero:
    entries nothing reaches (M == 0) are +0, bit for bit (without it they are 0 of either sign, by the bound itself)"""
    got64 = np.asarray(got, np.float64)
    assert got64.shape == ref.shape and np.isfinite(got64).all(), label
    err = np.abs(got64 - ref)
    reached = M > 0
    worst = float((err[reached] / (tol * M[reached])).max())
    sens = float(np.mean(near)) if near is not None else 0.0
    name = "%s %dx%d spp %d" % case if case else "model"
    print(f"{label} {name}: {reached.sum()} of {M.size} entries reached, {sens:.2%} of the pixels float32-sensitive; "
          f"worst error / ({tol:.4g} M) = {worst:.3g}")
    rep = os.environ.get("COR_F64_REPORT")
    if rep:
        with open(rep, "a") as fh:
            fh.write(json.dumps({"case": f"{label} {name}", "entries": int(M.size), "sensitive_frac": round(sens, 5),
                                 "tol": tol, "worst_ratio": worst}) + "\n")
    if plus_zero:
        assert not u32(np.ascontiguousarray(got, np.float32))[~reached].any(), label
    assert (err <= tol * M).all(), f"{label}: worst error / ({tol:.4g} M) = {worst:.3g}"
    if most:
        assert reached.sum() > M.size // 4, label
    return worst


# ------------------------------------------------------------------------------------------------ model_covariance
def edge_model():
    """the scene's rotations and scales, and six rows more: an unnormalised quaternion, a zero quaternion, one zero scale
    component, scales of 1e-6, of 1e3, and both in one row"""
    _, r, s, _, _ = S.scene()
    r2 = np.array([[0.9, -0.7, 0.4, 1.3], [0, 0, 0, 0], r[0], r[1], r[2], r[3]], np.float32)
    s2 = np.array([s[4], s[5], [s[0, 0], 0.0, s[0, 2]], [1e-6] * 3, [1e3] * 3, [1e-6, 1e3, 1.0]], np.float32)
    return np.concatenate([r, r2]), np.concatenate([s, s2])


def test_model_covariance_forward(ctx):
    import torch

    from gsrt.autograd import model_covariance

    r, s = edge_model()
    n = len(r)
    want = Q.cov6(F.covariance(r, s))
    M = Q.covariance_magnitude(r, s)
    got = model_covariance(torch.from_numpy(r).to("cuda:0"), torch.from_numpy(s).to("cuda:0")).cpu().numpy()
    sc = gsrt.Scene.from_model(ctx, np.zeros((n, 3), np.float32), r, s, np.full(n, 0.5, np.float32))
    try:
        built = sc.download()[0][:, 4:10]
    finally:
        sc.close()
    assert got.shape == (n, 6) and got.dtype == np.float32
    for label, a in (("model_covariance", got), ("k_cov3d", built)):
        hold(label + " forward", None, None, a, want, M, N_FWD * EPS, plus_zero=False)
    # the zero quaternion: R = I, Sigma = diag(s^2) as the formulas give it; a zero scale drops its row of R
    zq = S.N + 1
    for a in (got, built):
        assert not a[zq, [1, 2, 4]].any() and np.array_equal(a[zq, [0, 3, 5]], s[zq] * s[zq])
    assert (np.abs(want[S.N + 2]) > 0).all() and (np.abs(want[S.N + 4]) > 1e4).any() and (want[S.N + 3, [0, 3, 5]] < 1e-11).all()


def test_model_covariance_backward(ctx):
    """torch.autograd.grad of <cov, dcov> against param_chain, random float32 dcov: within N_TORCH 2^-24 M_scale / M_rot.
    At the zero quaternion every dR/dq is 0: rot's gradient is 0 there, and the bound (M_rot = 0) demands it."""
    import torch

    from gsrt.autograd import model_covariance

    r, s = edge_model()
    dcov = np.random.default_rng(61).uniform(-1.0, 1.0, (len(r), 6)).astype(np.float32)
    t_r = torch.from_numpy(r).to("cuda:0").requires_grad_(True)
    t_s = torch.from_numpy(s).to("cuda:0").requires_grad_(True)
    cov = model_covariance(t_r, t_s)
    g_r, g_s = torch.autograd.grad((cov * torch.from_numpy(dcov).to("cuda:0")).sum(), (t_r, t_s))
    d64 = dcov.astype(np.float64)
    ref = Q.param_chain(r, s, d64, np.abs(d64))
    assert not ref.M_rot[S.N + 1].any() and (ref.M_rot[:S.N] > 0).all() and (ref.M_scale[:S.N + 2] > 0).all()
    hold("model_covariance backward scale", None, None, g_s.cpu().numpy(), ref.scale, ref.M_scale, SQ.N_TORCH["scale"] * EPS,
         plus_zero=False)
    hold("model_covariance backward rot", None, None, g_r.cpu().numpy(), ref.rot, ref.M_rot, SQ.N_TORCH["rot"] * EPS,
         plus_zero=False)


# ------------------------------------------------------------------------------------------------ render_model
def run_model(ctx, monkeypatch, case, depth, sh_form="n163", loss=None):
    """One render_model and backward on the scene's tensors. sh_form: "n163", "n48", "none" (sh=None) or "frozen" (given,
    requires no gradient). loss(rgba, depth_or_None) -> scalar; default <G, rgba> (+ <Gdepth, depth>) of the case's cached
    upstream gradients. Returns grads (name -> numpy or None; "cov" the hooked cov3d gradient), rgba and rgba.grad."""
    import torch

    import gsrt.autograd as A

    c, r, s, o, sh = S.scene()
    ubo = TG.camera(case)
    seen = []
    plain_cov = A.model_covariance

    def hooked(rot, scale):
        cov = plain_cov(rot, scale)
        cov.register_hook(lambda g: seen.append(g.detach().clone()))
        return cov

    monkeypatch.setattr(A, "model_covariance", hooked)
    t = {k: torch.from_numpy(a).to("cuda:0").requires_grad_(True) for k, a in dict(c=c, r=r, s=s, o=o).items()}
    if sh_form == "none":
        t_sh = None
    else:
        t_sh = torch.from_numpy(sh.reshape(S.N, 48) if sh_form == "n48" else sh).to("cuda:0")
        t_sh.requires_grad_(sh_form != "frozen")
    if loss is None:
        ref = TD.reference(case, True) if depth else TQ.reference(case, True)
        d_G = torch.from_numpy(np.ascontiguousarray(ref[0])).to("cuda:0")
        d_Gd = torch.from_numpy(np.ascontiguousarray(ref[1])).to("cuda:0") if depth else None
        loss = lambda rgba, dep: (rgba * d_G).sum() + ((dep * d_Gd).sum() if depth else 0.0)  # noqa: E731
    # the scene render_model drives: built from other values, so that what it renders is what the forward put there
    sc = gsrt.Scene.from_model(ctx, c + np.float32(0.05), r, s * np.float32(1.1), o * np.float32(0.5), sh)
    try:
        sc.build_bvh()
        out = A.render_model(sc, ubo, t["c"], t["r"], t["s"], t["o"], t_sh, depth=depth)
        rgba, dep = out if depth else (out, None)
        rgba.retain_grad()
        value = loss(rgba, dep)
        value.backward()
        grads = {k: v.grad.cpu().numpy() for k, v in t.items()}
        grads["sh"] = None if t_sh is None or t_sh.grad is None else t_sh.grad.cpu().numpy()
        assert len(seen) == 1
        grads["cov"] = seen[0].cpu().numpy()
        up = None if rgba.grad is None else rgba.grad.cpu().numpy()
        return grads, rgba.detach().cpu().numpy(), up, value.detach().cpu().numpy()
    finally:
        sc.close()


def hold_model(label, case, depth, grads, rows, table=None):
    """the gradients of one backward against float64: rows = splat_gradients' / depth_gradients' result for the upstream
    gradients of that backward, table = F.gradients' for the same G (the SH table; None: sh.grad is not held here)"""
    c, r, s, o, _ = S.scene()
    ubo = TG.camera(case)
    c64, cov64 = c.astype(np.float64), Q.cov6(F.covariance(r, s))
    chain = D.depth_chain if depth else Q.model_chain
    ch, mm = chain(ubo, c64, cov64, rows.rows), chain(ubo, c64, cov64, rows.M)
    tol = SQ.model_tol(TD.CHAIN_OPS if depth else TQ.CHAIN_OPS)
    assert grads["cov"].shape == (S.N, 6) and grads["c"].shape == (S.N, 3)
    hold(label + " cov3d", case, rows.near, grads["cov"], ch.cov, mm.M2_cov, tol)
    hold(label + " center", case, rows.near, grads["c"], ch.center, mm.M2_center, tol)
    pc = Q.param_chain(r, s, ch.cov, mm.M2_cov)
    hold(label + " scale", case, rows.near, grads["s"], pc.scale, pc.M_scale, tol + SQ.N_TORCH["scale"] * EPS, plus_zero=False)
    hold(label + " rot", case, rows.near, grads["r"], pc.rot, pc.M_rot, tol + SQ.N_TORCH["rot"] * EPS, plus_zero=False)
    TG.hold(label + " opacity", case, rows.near, grads["o"], rows.rows[:, 5], rows.M[:, 5])
    if table is not None:
        TG.hold(label + " sh", case, rows.near, grads["sh"].reshape(table.sh.shape), table.sh, table.M_sh)


def cached(case, depth):
    return TD.reference(case, True)[2] if depth else TQ.reference(case, True)[1]


@DEPTH
@CASES
def test_every_gradient_matches_f64(ctx, monkeypatch, case, depth):
    grads, _, up, _ = run_model(ctx, monkeypatch, case, depth)
    assert up.tobytes() == np.ascontiguousarray(TG.reference(case, True)[0]).tobytes()  # the upstream gradient is G itself
    assert grads["sh"].shape == (S.N, 16, 3)
    hold_model("render_model depth" if depth else "render_model", case, depth, grads, cached(case, depth),
               TG.reference(case, True)[1])


@DEPTH
@pytest.mark.parametrize("sh_form", ["n48", "none", "frozen"])
def test_sh_forms(ctx, monkeypatch, depth, sh_form):
    """sh as (n, 48): its gradient comes back in that shape and is held; sh=None (the scene keeps its rows) and sh that
    requires no gradient: none is returned, and the other four are held to float64 as before (two backwards differ by their
    float atomics only, which the bounds cover)."""
    case = S.CASES[0]
    grads, _, _, _ = run_model(ctx, monkeypatch, case, depth, sh_form)
    label = f"render_model {'depth ' if depth else ''}sh {sh_form}"
    if sh_form == "n48":
        assert grads["sh"].shape == (S.N, 48)
        hold_model(label, case, depth, grads, cached(case, depth), TG.reference(case, True)[1])
    else:
        assert grads["sh"] is None
        hold_model(label, case, depth, grads, cached(case, depth))


def test_depth_alone(ctx, monkeypatch):
    """a loss of the depth only: rgba's upstream gradient is None in the backward and counts as zeros; held to
    depth_gradients with G = 0. The SH table gets no gradient or zeros."""
    import torch

    case = S.CASES[-1]
    _, w, h, _ = case
    c, r, s, o, sh = S.scene()
    Gd = TD.reference(case, True)[1]
    d_Gd = torch.from_numpy(np.ascontiguousarray(Gd)).to("cuda:0")
    grads, _, up, _ = run_model(ctx, monkeypatch, case, True, loss=lambda rgba, dep: (dep * d_Gd).sum())
    assert up is None
    dg = D.depth_gradients(TG.camera(case), c, r, s, o, sh, G_rgba=np.zeros((h, w, 4)), G_depth=Gd)
    hold_model("render_model depth alone", case, True, grads, dg)
    assert grads["sh"] is None or not grads["sh"].any()


def test_training_step_matches_f64(ctx, monkeypatch):
    """render_model -> photometric_loss (lam 0.2, a smooth target) -> backward on CASES[0]. Frame and target are multiplied
    by a 0 / 1 mask that is zero on the reference's float32-sensitive pixels, so the upstream gradient is zero there. The
    loss and rgba.grad have the bits of gsrt.image_loss of the downloaded masked frame (the upstream scalar is exactly 1),
    and the five parameter gradients are held to the float64 references fed rgba.grad itself."""
    import torch

    from gsrt.autograd import photometric_loss

    case = S.CASES[0]
    _, W, H, _ = case
    c, r, s, o, sh = S.scene()
    near = TQ.reference(case, True)[1].near
    assert 0 < near.sum() < near.size // 4
    mask = (~near).astype(np.float32)[..., None]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    target = np.stack([0.5 + 0.4 * np.sin(0.3 * xx), 0.5 + 0.4 * np.cos(0.2 * yy), 0.5 + 0.0 * xx], -1).astype(np.float32)
    target_m = target * mask
    d_mask, d_target = torch.from_numpy(mask).to("cuda:0"), torch.from_numpy(target_m).to("cuda:0")
    kept = {}

    def loss(rgba, _):
        kept["masked"] = rgba * d_mask
        return photometric_loss(ctx, kept["masked"], d_target, lam=0.2)

    grads, _, up, value = run_model(ctx, monkeypatch, case, False, loss=loss)
    want, gwant = gsrt.image_loss(ctx, kept["masked"].detach().cpu().numpy(), target_m, 0.2)
    assert value.dtype == np.float32 and value.view(np.uint32) == np.float32(want["loss"]).view(np.uint32)
    assert np.isfinite(want["loss"]) and want["loss"] > 0.0
    assert up.shape == (H, W, 4) and u32(up).tobytes() == u32(gwant * mask).tobytes()
    assert not up[near].any() and up[~near][:, :3].any() and not up[..., 3].any()
    G = up.astype(np.float64)
    ubo = TG.camera(case)
    sg = Q.splat_gradients(ubo, c, r, s, o, sh, G_rgba=G)
    assert np.array_equal(sg.near, near)
    hold_model("training step", case, False, grads, sg, F.gradients(ubo, c, r, s, o, sh, G_rgba=G))
