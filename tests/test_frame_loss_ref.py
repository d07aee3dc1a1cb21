"""The numpy reference of the frame loss (tests/frame_loss_ref.py) checked on its own, in float64: with no option it is
image_loss_ref.image_loss exactly, and its two analytic gradients agree with central differences of its own loss, for
every option alone and all together, at 5 x 7 (every entry of rgba, alpha included, and of depth) and at 17 x 33 (the
entries of 40 pixels, the corners among them, and two dense random directions). No device needed.

Central differences as in tests/test_image_loss_ref.py: the five-point stencil with h = 1e-3, held to 1e-9 of the largest
gradient entry. The inputs stay away from the kinks: |x' - y'| >= 0.3 * 0.02 = 0.006 > 2h under the smallest mask weight
(a step of alpha moves x by at most 2h as well), |e| >= 0.05, alpha in [0.5, 1] (far from alpha_min, and D / alpha's fifth
derivative 120 D / alpha^6 stays below 1e4, a truncation error of 3e-10 times depth_weight / (H W)), and the set of depth
samples (a finite positive target depth) does not depend on what is perturbed.
"""
import numpy as np
import pytest

import frame_loss_ref as F
import image_loss_ref as R

BG = (1.0, 0.25, 0.5)
OPTIONS = {"mask": dict(mask=True), "background": dict(background=True), "depth": dict(depth=True),
           "all": dict(mask=True, background=True, depth=True)}


def inputs(W, H, mask=False, background=False, depth=False):
    rng = np.random.default_rng(100 * W + H)
    rgba = rng.uniform(0.0, 1.0, (H, W, 4))
    rgba[..., 3] = rng.uniform(0.5, 1.0, (H, W))
    kw = {}
    x = rgba[..., :3]
    if background:
        kw["background"] = BG
        x = x + (1.0 - rgba[..., 3:]) * np.array(BG)
    target = x + rng.uniform(0.02, 0.2, (H, W, 3)) * rng.choice([-1.0, 1.0], (H, W, 3))
    if mask:
        kw["mask"] = rng.uniform(0.3, 1.0, (H, W))
    D = None
    if depth:
        z = rng.uniform(1.0, 4.0, (H, W))
        D = z * rgba[..., 3]
        t = z + rng.uniform(0.05, 0.5, (H, W)) * rng.choice([-1.0, 1.0], (H, W))
        t.flat[::5] = np.array([0.0, -1.0, np.nan, np.inf])[np.arange(t.flat[::5].size) % 4]  # no samples
        kw.update(target_depth=t, depth_weight=0.5)
    return rgba, target, D, kw


def loss_of(rgba, target, D, kw, lam):
    return F.frame_loss(rgba, target, lam, depth=D, want_grad=False, **kw)["loss"]


def stencil(f, h):
    return (f(-2 * h) - 8 * f(-h) + 8 * f(h) - f(2 * h)) / (12 * h)


@pytest.mark.parametrize("shape", [(5, 7), (17, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_no_option_is_image_loss(shape):
    W, H = shape
    rgba, target, _, _ = inputs(W, H)
    rgba[0, 0, 3] = np.nan  # not read
    for dtype in (np.float64, np.float32):
        a, b = F.frame_loss(rgba, target, 0.2, dtype), R.image_loss(rgba, target, 0.2, dtype)
        for k in ("loss", "l1", "ssim", "mse"):
            assert a[k] == b[k], k
        assert np.array_equal(a["grad"], b["grad"]) and np.array_equal(a["map"], b["map"])
        assert a["grad_depth"] is None and a["depth_l1"] == 0.0 and a["depth_samples"] == 0


@pytest.mark.parametrize("option", list(OPTIONS))
@pytest.mark.parametrize("shape", [(5, 7), (17, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_gradients_match_central_differences(shape, option):
    W, H = shape
    lam, h = 0.2, 1e-3
    rgba, target, D, kw = inputs(W, H, **OPTIONS[option])
    ref = F.frame_loss(rgba, target, lam, depth=D, **kw)
    g, gd = ref["grad"], ref["grad_depth"]
    if D is not None:
        assert 0 < ref["depth_samples"] < W * H and ref["depth_l1"] > 0.0
        assert not gd[~ref["sample"]].any()
    if "background" not in kw and D is None:
        assert not g[..., 3].any()

    def at(arr_is_depth, idx):
        def f(step):
            x, d = rgba.copy(), None if D is None else D.copy()
            (d if arr_is_depth else x)[idx] += step
            return loss_of(x, target, d, kw, lam)
        return f

    rng = np.random.default_rng(7)
    pixels = list(np.ndindex(H, W))
    if W * H > 40:
        keep = {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}
        keep |= {pixels[i] for i in rng.choice(len(pixels), 36, replace=False)}
        pixels = sorted(keep)
    scale = max(np.abs(g).max(), 0.0 if gd is None else np.abs(gd).max())
    err = 0.0
    for p in pixels:
        for c in range(4):
            err = max(err, abs(stencil(at(False, p + (c,)), h) - g[p + (c,)]))
        if D is not None:
            err = max(err, abs(stencil(at(True, p), h) - gd[p]))
    # dense directions: every entry moves at once, by at most h
    for _ in range(2):
        vx = rng.uniform(-1.0, 1.0, rgba.shape)
        vd = None if D is None else rng.uniform(-1.0, 1.0, D.shape)
        want = float((g * vx).sum()) + (0.0 if D is None else float((gd * vd).sum()))
        got = stencil(lambda s: loss_of(rgba + s * vx, target, None if D is None else D + s * vd, kw, lam), h / 2)
        err_dir = abs(got - want)
        print(f"{option} {W}x{H}: direction |fd - g.v| {err_dir:.3g} of {abs(want):.3g}")
        assert err_dir <= 1e-9 * scale * np.sqrt(vx.size)
    print(f"{option} {W}x{H}: max |fd - grad| {err:.3g}, max |grad| {scale:.3g}")
    assert err <= 1e-9 * scale
