"""The photometric loss on the GPU (gsrt_image_loss, gsrt_image_loss_async, gsrt.image_loss, gsrt.autograd.photometric_loss
and image_metrics) against the numpy reference of tests/image_loss_ref.py in float64. The reference is checked on the CPU
in tests/test_image_loss_ref.py.

Shapes (W x H), for a kernel with tiles of 32 x 16 pixels and a 5-pixel halo: 1 x 1; 5 x 7 (the window overhangs on every
side); 11 x 11; 16 x 16; 17 x 33 (three tile rows, the last with one row); 70 x 37 (three tile columns and rows: halos
cross two tile borders each way); 1 x 70 and 70 x 1; 64 x 64 (whole tiles only); and MANY_TILES, past one trip of the
scalar reduction's loop, up to the accepted limits of 32768 each way.

Inputs: smooth fields in [0, 1] plus noise, the target the frame plus a perturbation, and, by fractions of the image so
that every shape has them: a block where target == frame exactly (sign(0)), a flat block of two constants (the variances
cancel to about 0 and C2 governs), a block scaled outside [0, 1] (no clamp), and alpha (the target's fourth channel too)
filled with large values, infinities and NaNs (not read).

Tolerances. The gradient, per case: 8 max |ref32 - ref64| over the image, ref32 the same reference run in float32: the
rounding of float32 arithmetic on this input, with a factor for the different summation order (two 1-D passes against
121 taps). ssim: 8 max |map32 - map64|. l1 and mse: 2^-20 relative (per term one rounded subtraction and one rounded
square, the sum in double, one final rounding: 3 x 2^-24 at most). loss: (1 - lam) tol_l1 + lam tol_ssim plus 2^-23 |loss|
for its own rounding to float32.
"""
import ctypes
import functools

import numpy as np
import pytest

import gsrt
import image_loss_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 7), (11, 11), (16, 16), (17, 33), (70, 37), (1, 70), (70, 1), (64, 64)]
LAMBDAS = [0.0, 0.2, 1.0]
# W x H of more than 256 tiles, so that a lane of k_loss_scalars adds a second partial sum (lam 0.2 only): 1 x 4097 is 257
# tiles (lane 0 alone takes two), 530 x 260 is 17 x 17 = 289, ragged both ways, and the accepted limits, 32768 x 1 (1024
# tiles) and 1 x 32768 (2048)
MANY_TILES = [(1, 4097), (530, 260), (32768, 1), (1, 32768)]


@functools.lru_cache(maxsize=None)
def images(W, H, channels):
    """(rgba, target, same): the inputs of a shape, and the mask of pixels where target == frame exactly"""
    rng = np.random.default_rng(1000 * W + H)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    x = np.stack([0.5 + 0.4 * np.sin(0.11 * (c + 1) * xx + 0.5 * c) * np.cos(0.07 * (c + 2) * yy) for c in range(3)], -1)
    x = np.clip(x + rng.normal(0.0, 0.05, x.shape), 0.0, 1.0)
    y = np.clip(x + rng.normal(0.0, 0.05, x.shape) + 0.03 * np.sin(0.3 * xx + 0.2 * yy)[..., None], 0.0, 1.0)

    def block(fy0, fy1, fx0, fx1):  # at least one pixel, whatever the shape
        y0, x0 = int(fy0 * H), int(fx0 * W)
        return slice(y0, max(y0 + 1, int(fy1 * H))), slice(x0, max(x0 + 1, int(fx1 * W)))
    flat = block(0.55, 0.9, 0.05, 0.45)
    x[flat], y[flat] = (0.6, 0.3, 0.8), (0.55, 0.35, 0.8)
    wide = block(0.5, 1.0, 0.55, 1.0)
    x[wide] = 1.6 * x[wide] - 0.3
    y[wide] = 1.5 * y[wide] - 0.2
    same = np.zeros((H, W), bool)
    same[block(0.1, 0.45, 0.1, 0.5)] = True
    same[flat], same[wide] = False, False  # where the blocks of a small shape meet, the other two stay
    y[same] = x[same]
    junk = np.array([1e30, -1e30, np.inf, -np.inf, np.nan, 7.0], np.float32)
    rgba = np.concatenate([x.astype(np.float32), rng.choice(junk, (H, W, 1))], -1)
    target = y.astype(np.float32)
    if channels == 4:
        target = np.concatenate([target, rng.choice(junk, (H, W, 1))], -1)
    target[same, :3] = rgba[same, :3]
    rgba.setflags(write=False)
    target.setflags(write=False)
    return rgba, target, same


@functools.lru_cache(maxsize=None)
def reference(W, H, channels, lam):
    rgba, target, _ = images(W, H, channels)
    return R.image_loss(rgba, target, lam, np.float64), R.image_loss(rgba, target, lam, np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scalars(d):
    return np.array([d["loss"], d["l1"], d["ssim"], d["mse"]], np.float32)


@pytest.mark.parametrize("shape,channels,lam", [(s, c, lam) for lam in LAMBDAS for c in (3, 4) for s in SHAPES] +
                         [(s, c, 0.2) for c in (3, 4) for s in MANY_TILES],
                         ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v))
def test_matches_reference(ctx, shape, channels, lam):
    W, H = shape
    rgba, target, same = images(W, H, channels)
    r64, r32 = reference(W, H, channels, lam)
    out, grad = gsrt.image_loss(ctx, rgba, target, lam)
    assert grad.dtype == np.float32 and grad.shape == (H, W, 4)

    tol_g = 8.0 * float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max())
    err_g = float(np.abs(grad[..., :3].astype(np.float64) - r64["grad"][..., :3]).max())
    tol_s = 8.0 * float(np.abs(r32["map"].astype(np.float64) - r64["map"]).max())
    err_s = abs(out["ssim"] - r64["ssim"])
    print(f"image_loss {W}x{H} c{channels} lam {lam}: grad err {err_g:.3e} ref32 {tol_g / 8:.3e} max |grad| "
          f"{np.abs(r64['grad']).max():.3e}; ssim err {err_s:.3e} map32 {tol_s / 8:.3e}; l1 err "
          f"{abs(out['l1'] - r64['l1']):.3e} of {r64['l1']:.3e}, mse err {abs(out['mse'] - r64['mse']):.3e} of {r64['mse']:.3e}")
    assert np.isfinite(grad).all()
    assert not bits(grad[..., 3]).any()  # +0 bitwise
    assert err_g <= tol_g
    if lam == 0.0:
        assert not grad[same].any()
    tol_l1, tol_mse = 2.0 ** -20 * r64["l1"], 2.0 ** -20 * r64["mse"]
    assert abs(out["l1"] - r64["l1"]) <= tol_l1
    assert abs(out["mse"] - r64["mse"]) <= tol_mse
    assert err_s <= tol_s
    assert abs(out["loss"] - r64["loss"]) <= (1 - lam) * tol_l1 + lam * tol_s + 2.0 ** -23 * abs(r64["loss"])


@pytest.mark.parametrize("shape", [(5, 7), (70, 37)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_deterministic_and_no_gradient(ctx, shape):
    """the same call twice: the same bits; without a gradient: the same scalars"""
    W, H = shape
    rgba, target, _ = images(W, H, 3)
    a, ga = gsrt.image_loss(ctx, rgba, target, 0.2)
    b, gb = gsrt.image_loss(ctx, rgba, target, 0.2)
    c, gc = gsrt.image_loss(ctx, rgba, target, 0.2, want_grad=False)
    assert gc is None
    assert np.array_equal(bits(scalars(a)), bits(scalars(b))) and np.array_equal(bits(scalars(a)), bits(scalars(c)))
    assert np.array_equal(bits(ga), bits(gb))


@pytest.mark.parametrize("channels", [3, 4])
def test_device_pointers_match_host_pointers(ctx, channels):
    """device tensors through the blocking call and through gsrt_image_loss_async: the bits of the host path"""
    import torch

    W, H = 70, 37
    rgba, target, _ = images(W, H, channels)
    want, gwant = gsrt.image_loss(ctx, rgba, target, 0.2)
    x, y = torch.from_numpy(rgba.copy()).to("cuda:0"), torch.from_numpy(target.copy()).to("cuda:0")
    g = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    got = gsrt.image_loss(ctx, x.data_ptr(), y.data_ptr(), 0.2, width=W, height=H, target_channels=channels,
                          d_grad=g.data_ptr())
    assert np.array_equal(bits(scalars(got)), bits(scalars(want)))
    assert np.array_equal(bits(g.cpu().numpy()), bits(gwant))
    out = torch.zeros(4, dtype=torch.float32, device="cuda:0")
    g.fill_(7.0)
    torch.cuda.synchronize()
    assert gsrt.image_loss(ctx, x.data_ptr(), y.data_ptr(), 0.2, width=W, height=H, target_channels=channels,
                           d_out=out.data_ptr(), d_grad=g.data_ptr(), asynchronous=True) is None
    ctx.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(scalars(want)))
    assert np.array_equal(bits(g.cpu().numpy()), bits(gwant))


def test_workspace_regrows(ctx):
    """A context's loss workspace grows on demand (a stream synchronise first, then the derivative maps lie at another
    offset): on contexts of their own, a small frame with a gradient, a larger one without (fits), the same with one
    (regrown), a still larger one (regrown), the small one again. Once through the blocking call and once through
    gsrt_image_loss_async on device tensors with no synchronise between the calls; every result has the bits of the shared
    context's result for that shape."""
    import torch

    order = [((5, 7), True), ((70, 37), False), ((70, 37), True), ((530, 260), True), ((5, 7), True)]
    want = {shape: gsrt.image_loss(ctx, *images(*shape, 3)[:2], 0.2) for shape, _ in order}
    own = gsrt.Context(0)
    try:
        for (W, H), with_grad in order:
            rgba, target, _ = images(W, H, 3)
            out, grad = gsrt.image_loss(own, rgba, target, 0.2, want_grad=with_grad)
            assert np.array_equal(bits(scalars(out)), bits(scalars(want[W, H][0]))), (W, H, with_grad)
            assert (grad is None) == (not with_grad)
            assert grad is None or np.array_equal(bits(grad), bits(want[W, H][1])), (W, H)
    finally:
        own.close()
    own = gsrt.Context(0)
    try:
        calls = []
        for (W, H), with_grad in order:
            rgba, target, _ = images(W, H, 3)
            calls.append((W, H, torch.from_numpy(rgba.copy()).to("cuda:0"), torch.from_numpy(target.copy()).to("cuda:0"),
                          torch.full((4,), 7.0, dtype=torch.float32, device="cuda:0"),
                          torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda:0") if with_grad else None))
        torch.cuda.synchronize()
        for W, H, x, y, out, grad in calls:
            assert gsrt.image_loss(own, x.data_ptr(), y.data_ptr(), 0.2, width=W, height=H, target_channels=3,
                                   d_out=out.data_ptr(), d_grad=grad.data_ptr() if grad is not None else 0,
                                   asynchronous=True) is None
        own.synchronize()
        for W, H, _, _, out, grad in calls:
            assert np.array_equal(bits(out.cpu().numpy()), bits(scalars(want[W, H][0]))), (W, H)
            assert grad is None or np.array_equal(bits(grad.cpu().numpy()), bits(want[W, H][1])), (W, H)
    finally:
        own.close()


def test_refusals_leave_outputs_untouched(ctx):
    import torch

    W, H = 5, 7
    rgba, target, _ = images(W, H, 4)
    rgba, target = rgba.copy(), target.copy()
    out = np.full(4, 3.0, np.float32)
    grad = np.full((H, W, 4), 3.0, np.float32)
    d_x = torch.from_numpy(rgba).to("cuda:0")
    d_y = torch.from_numpy(target).to("cuda:0")
    d_g = torch.full((H, W, 4), 3.0, dtype=torch.float32, device="cuda:0")
    d_o = torch.full((4,), 3.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    P = lambda a: ctypes.c_void_p(a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr())  # noqa: E731
    L, h = gsrt.lib, ctx.handle
    host = dict(width=W, height=H, rgba=P(rgba), target=P(target), channels=4, lam=0.2, out=P(out), grad=P(grad))

    def call(fn=L.gsrt_image_loss, **kw):
        a = dict(host, **kw)
        return fn(h, a["width"], a["height"], a["rgba"], a["target"], a["channels"], a["lam"], a["out"], a["grad"])
    assert call() == gsrt.OK  # the arguments the refusals below vary
    out[:], grad[:] = 3.0, 3.0
    refused = [dict(rgba=None), dict(target=None), dict(out=None), dict(width=0), dict(height=0), dict(width=32769),
               dict(height=32769), dict(channels=2), dict(channels=5), dict(channels=0), dict(lam=-0.01), dict(lam=1.01),
               dict(lam=float("nan")), dict(out=P(d_o)),
               dict(rgba=P(d_x)), dict(target=P(d_y)), dict(grad=P(d_g)), dict(rgba=P(d_x), target=P(d_y)),
               dict(grad=P(rgba)), dict(grad=P(target)),
               dict(grad=ctypes.c_void_p(rgba.ctypes.data + 16 * (W * H - 1)))]  # overlaps the last pixel
    for kw in refused:
        assert call(**kw) == gsrt.E_ARG, kw
        assert (out == 3.0).all() and (grad == 3.0).all(), kw
    assert L.gsrt_image_loss(None, W, H, P(rgba), P(target), 4, 0.2, P(out), P(grad)) == gsrt.E_ARG
    dev = dict(rgba=P(d_x), target=P(d_y), out=P(d_o), grad=P(d_g))
    for kw in (dict(rgba=None), dict(target=None), dict(out=None), dict(width=0), dict(channels=1), dict(lam=2.0),
               dict(lam=float("nan")), dict(grad=P(d_x)), dict(grad=P(d_y))):
        assert call(L.gsrt_image_loss_async, **dict(dev, **kw)) == gsrt.E_ARG, kw
    ctx.synchronize()
    assert (out == 3.0).all() and (grad == 3.0).all()
    assert (d_o == 3.0).all().item() and (d_g == 3.0).all().item()
    with pytest.raises(gsrt.GsrtError):
        gsrt.image_loss(ctx, rgba[:, :, :3], target)


def test_photometric_loss_autograd(ctx):
    """a leaf rgba: rgba.grad is gsrt.image_loss's gradient times the upstream scalar; image_metrics: the same scalars"""
    import torch

    from gsrt.autograd import image_metrics, photometric_loss

    W, H = 70, 37
    rgba, target, _ = images(W, H, 3)
    rgba = np.array(rgba)
    rgba[..., 3] = 1.0  # the upstream product below must be finite
    want, gwant = gsrt.image_loss(ctx, rgba, target, 0.2)
    x = torch.from_numpy(rgba).to("cuda:0").requires_grad_(True)
    y = torch.from_numpy(np.array(target)).to("cuda:0")
    loss = photometric_loss(ctx, x, y, lam=0.2)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert np.float32(loss.item()).view(np.uint32) == np.float32(want["loss"]).view(np.uint32)
    (loss * 2.5).backward()
    assert np.array_equal(bits(x.grad.cpu().numpy()), bits(np.float32(2.5) * gwant))
    m = image_metrics(ctx, x.detach(), y)
    assert np.array_equal(bits(scalars(m)), bits(scalars(want)))
    assert m["psnr"] == pytest.approx(-10.0 * np.log10(want["mse"]))


def test_render_model_to_loss_backward(ctx):
    """render_model -> photometric_loss -> backward on the small model of tests/test_grad_f64.py: every parameter gets a
    finite gradient that is not all zero"""
    import torch

    import test_grad_f64 as S
    import test_grad_f64_gpu as TG
    from gsrt.autograd import photometric_loss, render_model

    case = S.CASES[0]
    _, W, H, _ = case
    c, r, s, o, sh = S.scene()
    ubo = TG.camera(case)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        target = np.stack([0.5 + 0.4 * np.sin(0.3 * xx), 0.5 + 0.4 * np.cos(0.2 * yy), 0.5 + 0.0 * xx], -1).astype(np.float32)
        t = {k: torch.from_numpy(a).to("cuda:0").requires_grad_(True) for k, a in dict(c=c, r=r, s=s, o=o, sh=sh).items()}
        rgba = render_model(sc, ubo, t["c"], t["r"], t["s"], t["o"], t["sh"])
        loss = photometric_loss(ctx, rgba, torch.from_numpy(target).to("cuda:0"))
        assert np.isfinite(loss.item()) and loss.item() > 0.0
        loss.backward()
        for k, v in t.items():
            assert v.grad is not None and v.grad.shape == v.shape, k
            assert torch.isfinite(v.grad).all().item(), k
            assert (v.grad != 0).any().item(), k
    finally:
        sc.close()
