"""numpy reference of the frame loss (gsrt_frame_loss, include/gsrt.h): the photometric loss of a frame composited over a
background, under a pixel mask, plus a depth term, and the analytic gradients with respect to the frame (alpha included)
and to its premultiplied depth.

A restatement of the header's formulas in a chosen dtype: float64 is the reference, float32 the rounding yardstick of the
GPU tests, with every operation rounded on its own in the header's order. The window sums, the SSIM map and its exact
derivative are image_loss_ref's (121-tap sums, nothing separable). What a C float holds (lambda aside, which
image_loss_ref converts itself) is rounded to float32 first in either dtype: the background, depth_weight, alpha_min.
"""
import numpy as np

import image_loss_ref as R


def frame_loss(rgba, target, lam, dtype=np.float64, mask=None, depth=None, target_depth=None, background=None,
               depth_weight=0.0, alpha_min=1.0 / 255.0, want_grad=True):
    """rgba (H, W, 4), target (H, W, 3 or 4), mask / depth / target_depth (H, W) or None, background (r, g, b) or None
    -> dict(loss, l1, ssim, mse, depth_l1, depth_samples, map, sample[, grad (H, W, 4), grad_depth (H, W) or None]) computed
    in `dtype` (the scalars are sums taken in float64 of the dtype's per-pixel terms, as the kernel sums in double)"""
    rgba = np.asarray(rgba)
    H, W = rgba.shape[:2]
    x = rgba[..., :3].astype(dtype)
    y = np.asarray(target)[..., :3].astype(dtype)
    a = rgba[..., 3].astype(dtype)
    m = None if mask is None else np.asarray(mask).astype(dtype)
    bg = None if background is None else np.asarray(background, np.float32).astype(dtype)
    if bg is not None:
        k = dtype(1) - a
        x = x + k[..., None] * bg
    if m is not None:
        x, y = m[..., None] * x, m[..., None] * y
    frame = np.concatenate([x, np.zeros((H, W, 1), dtype)], -1)
    out = R.image_loss(frame, y, lam, dtype, want_grad)
    dw = float(np.float32(depth_weight))
    sample = np.zeros((H, W), bool)
    out["depth_l1"], out["depth_samples"] = 0.0, 0
    if depth is not None:
        t32 = np.asarray(target_depth, np.float32)
        with np.errstate(invalid="ignore"):
            sample = np.isfinite(t32) & (t32 > 0) & (rgba[..., 3].astype(np.float32) >= np.float32(alpha_min))
        a_s = np.where(sample, a, dtype(1))
        q = np.where(sample, np.asarray(depth).astype(dtype), dtype(0)) / a_s
        e = np.where(sample, q - np.where(sample, t32, 0).astype(dtype), dtype(0))
        term = np.abs(e) if m is None else m * np.abs(e)
        out["depth_l1"] = float(np.where(sample, term, 0).astype(np.float64).sum() / (H * W))
        out["depth_samples"] = int(sample.sum())
        out["loss"] = out["loss"] + dw * out["depth_l1"]
    out["sample"] = sample
    if want_grad:
        g = out["grad"][..., :3]
        grad = np.zeros((H, W, 4), dtype)
        grad[..., :3] = g if m is None else m[..., None] * g
        if bg is not None:
            b = (g[..., 0] * bg[0] + g[..., 1] * bg[1]) + g[..., 2] * bg[2]
            grad[..., 3] = -(b if m is None else m * b)
        out["grad_depth"] = None
        if depth is not None:
            kd = dtype(dw / (H * W))
            s = (kd if m is None else kd * m) * np.sign(e)
            out["grad_depth"] = np.where(sample, s / a_s, dtype(0)).astype(dtype)
            grad[..., 3] = np.where(sample, grad[..., 3] - (s * q) / a_s, grad[..., 3])
        out["grad"] = grad
    return out
