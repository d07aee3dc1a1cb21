"""The numpy reference of the photometric loss (tests/image_loss_ref.py) checked on its own, in float64: its analytic
gradient against central differences of its own loss, and loss and gradient against 3DGS's formulation (conv2d with
padding 5 and groups 3, autograd) in torch float64 on the CPU, which shares no code with it. No device needed.

Both comparisons hold the gradient to 1e-9 of its largest entry. The image is 9 x 8, so every pixel is a border pixel:
each window overhangs the image and the zero padding is in every term.
Central differences: the five-point stencil (f(-2h) - 8 f(-h) + 8 f(h) - f(2h)) / 12h with h = 1e-3. Its truncation
error is h^4 f^(5) / 30 = 3e-14 f^(5), and one pixel moves a window mean by at most 0.0708 h (the largest 2-D weight), so
the loss is smooth on that scale for a textured image (variances far above C2); the rounding of the loss (about 1e-16 of
a value near 0.3) over 12h contributes about 1e-14. The largest gradient entry is about 1e-2, so 1e-9 of it is 1e-11.
|x - y| >= 0.01 > 2h everywhere, so no step crosses the kink of the L1 term.
"""
import numpy as np
import pytest
import torch

import image_loss_ref as R

W, H = 9, 8


def images(channels=3):
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)
    step = rng.uniform(0.01, 0.2, (H, W, channels)) * rng.choice([-1.0, 1.0], (H, W, channels))
    y = (x[..., :channels] + step).astype(np.float32)
    return x, y


def test_window():
    w = R.window()
    assert w.dtype == np.float32 and w.shape == (11,)
    assert np.array_equal(w, w[::-1]) and w.argmax() == 5
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23


@pytest.mark.parametrize("lam", [0.2, 1.0])
def test_gradient_matches_central_differences(lam):
    x, y = images()
    x = x.astype(np.float64)
    assert np.abs(x[..., :3] - y).min() >= 0.0099
    g = R.image_loss(x, y, lam)["grad"]
    assert not g[..., 3].any()
    h = 1e-3
    fd = np.zeros((H, W, 3))
    for idx in np.ndindex(H, W, 3):
        f = []
        for k in (-2, -1, 1, 2):
            xp = x.copy()
            xp[idx] += k * h
            f.append(R.image_loss(xp, y, lam, want_grad=False)["loss"])
        fd[idx] = (f[0] - 8 * f[1] + 8 * f[2] - f[3]) / (12 * h)
    err = np.abs(fd - g[..., :3]).max()
    print(f"lam {lam}: max |fd - grad| {err:.3g}, max |grad| {np.abs(g).max():.3g}")
    assert err <= 1e-9 * np.abs(g).max()


@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
def test_matches_3dgs_formulation(lam, channels):
    x, y = images(channels)
    ref = R.image_loss(x, y, lam)

    w = torch.from_numpy(R.window().astype(np.float64))
    win = (w[:, None] * w[None, :]).expand(3, 1, 11, 11).contiguous()
    tx = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    a = tx[..., :3].permute(2, 0, 1)[None]
    b = torch.from_numpy(y.astype(np.float64))[..., :3].permute(2, 0, 1)[None]
    conv = lambda t: torch.nn.functional.conv2d(t, win, padding=5, groups=3)  # noqa: E731
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 ** 2, conv(b * b) - mu2 ** 2, conv(a * b) - mu1 * mu2
    m = ((2 * mu1 * mu2 + R.C1) * (2 * s12 + R.C2)) / ((mu1 ** 2 + mu2 ** 2 + R.C1) * (s1 + s2 + R.C2))
    l1, ssim = (a - b).abs().mean(), m.mean()
    loss = (1 - lam) * l1 + lam * (1 - ssim)
    loss.backward()
    g = tx.grad.numpy()

    assert abs(ref["l1"] - l1.item()) <= 1e-12 and abs(ref["ssim"] - ssim.item()) <= 1e-12
    assert abs(ref["mse"] - ((a - b) ** 2).mean().item()) <= 1e-12 and abs(ref["loss"] - loss.item()) <= 1e-12
    err = np.abs(g - ref["grad"]).max()
    print(f"lam {lam}: max |torch - grad| {err:.3g}, max |grad| {np.abs(g).max():.3g}")
    assert err <= 1e-9 * np.abs(ref["grad"]).max()
    assert not ref["grad"][..., 3].any() and not g[..., 3].any()
