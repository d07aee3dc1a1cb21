"""numpy reference of the photometric loss (gsrt_image_loss, include/gsrt.h): L1 + D-SSIM of a frame against a target and
the analytic gradient with respect to the frame.

Every window sum is a direct 121-tap 2-D sum over an explicitly zero-padded image: nothing is separable here, so the
reference shares no structure with the kernel's two 1-D passes. It is dtype-generic: float64 is the reference, float32
the rounding yardstick of the GPU tests (the same formulas with every operation rounded to float32). Both use the float32
window table, so only rounding separates either from the kernel.
"""
import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2


def window() -> np.ndarray:
    """the 11 weights: exp(-(i - 5)^2 / (2 * 1.5^2)) normalised to sum 1 in float64, each rounded to float32 once"""
    i = np.arange(11, dtype=np.float64)
    w = np.exp(-((i - 5.0) ** 2) / (2.0 * 1.5 ** 2))
    return (w / w.sum()).astype(np.float32)


def _conv(img, dtype):
    """the 11 x 11 window over img (H, W, 3) padded with 5 zeros on every side: 121 taps, row-major"""
    w = window().astype(dtype)
    H, W = img.shape[:2]
    pad = np.zeros((H + 10, W + 10, img.shape[2]), dtype)
    pad[5:5 + H, 5:5 + W] = img
    out = np.zeros(img.shape, dtype)
    for dy in range(11):
        for dx in range(11):
            out += (w[dy] * w[dx]) * pad[dy:dy + H, dx:dx + W]
    return out


def image_loss(rgba, target, lam, dtype=np.float64, want_grad=True):
    """rgba (H, W, 4), target (H, W, 3 or 4) -> dict(loss, l1, ssim, mse, map[, grad (H, W, 4)]) computed in `dtype`
    (the scalars are means taken in float64 of the dtype's per-pixel terms, as the kernel sums in double)"""
    x = np.asarray(rgba)[..., :3].astype(dtype)
    y = np.asarray(target)[..., :3].astype(dtype)
    lam = dtype(lam)
    n = x.size
    d = x - y
    mu1, mu2 = _conv(x, dtype), _conv(y, dtype)
    s1 = _conv(x * x, dtype) - mu1 * mu1
    s2 = _conv(y * y, dtype) - mu2 * mu2
    s12 = _conv(x * y, dtype) - mu1 * mu2
    c1, c2 = dtype(C1), dtype(C2)
    a1, a2 = 2 * mu1 * mu2 + c1, 2 * s12 + c2
    b1, b2 = mu1 * mu1 + mu2 * mu2 + c1, s1 + s2 + c2
    m = (a1 * a2) / (b1 * b2)
    l1 = float(np.abs(d).astype(np.float64).mean())
    mse = float((d * d).astype(np.float64).mean())
    ssim = float(m.astype(np.float64).mean())
    out = dict(l1=l1, mse=mse, ssim=ssim, loss=(1.0 - float(lam)) * l1 + float(lam) * (1.0 - ssim), map=m)
    if want_grad:
        # map as a function of mu1, E[x^2] and E[xy] (s1 = E[x^2] - mu1^2, s12 = E[xy] - mu1 mu2); each of the three
        # window sums is linear in x with the symmetric window, so the chain back to x is the window over each partial
        dm_dmu1 = (2 * mu2 * (a2 - a1)) / (b1 * b2) - m * (2 * mu1 * (b2 - b1)) / (b1 * b2)
        dm_ds1 = -m / b2
        dm_ds12 = 2 * a1 / (b1 * b2)
        g_ssim = _conv(dm_dmu1, dtype) + 2 * x * _conv(dm_ds1, dtype) + y * _conv(dm_ds12, dtype)
        g = ((1 - lam) / dtype(n)) * np.sign(d) - (lam / dtype(n)) * g_ssim
        grad = np.zeros(x.shape[:2] + (4,), dtype)
        grad[..., :3] = g
        out["grad"] = grad
    return out
