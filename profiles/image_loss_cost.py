"""Time of the fused photometric loss (gsrt_image_loss_async: scalars and gradient) against the torch formulation a caller
would otherwise write, on the same GPU in the same process.

  python3 profiles/image_loss_cost.py [--width 1920 --height 1080 --rounds 7 --calls 50 --out FILE]

The torch formulation is 3DGS's, applied to the library's framebuffer layout: rgba[H, W, 4] -> permute to [1, 3, H, W],
five grouped 11 x 11 conv2d calls (padding 5), the elementwise SSIM map, 0.8 L1 + 0.2 (1 - SSIM), autograd's backward, and
the [H, W, 4] gradient as rgba.grad (the alpha slot zero): what gsrt_render_splat_grad takes.

Method: both are warmed up (10 calls each), then `rounds` rounds alternate the two; in a round each runs `calls` times
back to back between two device events on its own stream (the library's stream, torch's current stream), with a device
synchronise before and after, so a figure is device time per call including launch gaps, as a training step sees it.
Reported per variant: the median over rounds and the smallest and largest round. Same inputs for both; the two losses
and gradients are compared before timing (the torch one is float32 too, so they agree to rounding, not to the bit).
No GPU: the script fails, it does not fall back."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3dgs-raytrace_amd"))
import gsrt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--lam", type=float, default=0.2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("image_loss_cost: no GPU")
    W, H, lam = a.width, a.height, a.lam
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(0.011 * (c + 1) * xx) * torch.cos(0.007 * (c + 2) * yy) for c in range(4)], -1)
    rgba = (base + 0.05 * torch.randn(base.shape, generator=g)).clamp(0, 1).to(dev).contiguous()
    target = (rgba[..., :3].cpu() + 0.05 * torch.randn((H, W, 3), generator=g)).clamp(0, 1).to(dev).contiguous()

    ctx = gsrt.Context(0)
    d_out = torch.zeros(4, dtype=torch.float32, device=dev)
    d_grad = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    lib_stream = torch.cuda.ExternalStream(ctx.stream, device=dev)

    def fused():
        gsrt.image_loss(ctx, rgba.data_ptr(), target.data_ptr(), lam, width=W, height=H, target_channels=3,
                        d_out=d_out.data_ptr(), d_grad=d_grad.data_ptr(), asynchronous=True)

    w1 = torch.from_numpy(gsrt.image_loss_window()).to(dev)
    win = (w1[:, None] * w1[None, :]).expand(3, 1, 11, 11).contiguous()
    x = rgba.clone().requires_grad_(True)
    last = {}

    def torch_form():
        x.grad = None
        p = x[..., :3].permute(2, 0, 1)[None]
        q = target.permute(2, 0, 1)[None]
        conv = lambda t: torch.nn.functional.conv2d(t, win, padding=5, groups=3)  # noqa: E731
        mu1, mu2 = conv(p), conv(q)
        mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
        s1, s2, s12 = conv(p * p) - mu1_sq, conv(q * q) - mu2_sq, conv(p * q) - mu12
        m = ((2 * mu12 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
        loss = (1 - lam) * (p - q).abs().mean() + lam * (1 - m.mean())
        loss.backward()
        last["loss"] = loss.detach()

    for _ in range(10):
        fused()
        torch_form()
    ctx.synchronize()
    torch.cuda.synchronize()
    agree = dict(loss_fused=float(d_out[0]), loss_torch=float(last["loss"]),
                 grad_max_abs_diff=float((d_grad - x.grad).abs().max()), grad_max_abs=float(x.grad.abs().max()))

    def timed(fn, stream):
        ctx.synchronize()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            fn()
        e1.record(stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    ms = {"fused": [], "torch": []}
    for _ in range(a.rounds):
        ms["fused"].append(timed(fused, lib_stream))
        ms["torch"].append(timed(torch_form, torch.cuda.current_stream(dev)))
    res = dict(width=W, height=H, lam=lam, rounds=a.rounds, calls=a.calls, agree=agree)
    for k, v in ms.items():
        res[k + "_ms"] = dict(median=float(np.median(v)), min=min(v), max=max(v))
    res["torch_over_fused"] = res["torch_ms"]["median"] / res["fused_ms"]["median"]
    # the bytes the fused call must move at least: rgba and target read twice, nine planes written and read, gradient written
    px = W * H
    res["fused_min_bytes"] = px * 4 * (2 * (4 + 3) + 2 * 9 + 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
