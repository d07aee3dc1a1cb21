"""Time of the frame loss (gsrt_frame_loss_async: scalars and both gradients) beside the photometric loss it extends
(gsrt_image_loss_async), on the same GPU in the same process, on the same frame with a 3-channel target.

  python3 profiles/frame_loss_cost.py [--width 1920 --height 1080 --rounds 9 --calls 50 --out FILE]

Three variants: `all` (background, mask and depth term, grad_depth written), `none` (no option: the same arithmetic as
gsrt_image_loss in kernels of its own) and `image_loss` (gsrt_image_loss, whose kernels this library shares bit for bit
with the revision before the frame loss: DESIGN.md section 3 has the compiler's resource table).

Method, as profiles/image_loss_cost.py: all three are warmed up (10 calls each), then `rounds` rounds interleave them, the
order rotating by one each round; in a round a variant runs `calls` times back to back between two device events on the
library's stream, with a device synchronise before and after, so a figure is device time per call including launch
gaps, as a training step sees it. Reported per variant: the median over rounds and the smallest and largest round; the
spread of image_loss's rounds is the yardstick for `none`. The results are checked before timing: `none` has image_loss's
bits. No GPU: the script fails, it does not fall back."""
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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--lam", type=float, default=0.2)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_loss_cost: no GPU")
    W, H, lam = a.width, a.height, a.lam
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(1)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(0.011 * (c + 1) * xx) * torch.cos(0.007 * (c + 2) * yy) for c in range(4)], -1)
    rgba = (base + 0.05 * torch.randn(base.shape, generator=g)).clamp(0.05, 1).to(dev).contiguous()
    target = (rgba[..., :3].cpu() + 0.05 * torch.randn((H, W, 3), generator=g)).clamp(0, 1).to(dev).contiguous()
    mask = torch.rand((H, W), generator=g).to(dev).contiguous()
    z = 1.0 + 3.0 * torch.rand((H, W), generator=g)
    depth = (z.to(dev) * rgba[..., 3]).contiguous()
    target_depth = (z + 0.2 * torch.randn((H, W), generator=g)).to(dev).contiguous()

    ctx = gsrt.Context(0)
    out = {k: torch.zeros(6, dtype=torch.float32, device=dev) for k in ("all", "none", "image_loss")}
    grad = {k: torch.zeros((H, W, 4), dtype=torch.float32, device=dev) for k in out}
    d_gdepth = torch.zeros((H, W), dtype=torch.float32, device=dev)
    lib_stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
    dims = dict(width=W, height=H, target_channels=3, asynchronous=True)

    def run_all():
        gsrt.frame_loss(ctx, rgba.data_ptr(), target.data_ptr(), mask=mask.data_ptr(), depth=depth.data_ptr(),
                        target_depth=target_depth.data_ptr(), background=(1.0, 1.0, 1.0), lam=lam, depth_weight=0.5,
                        d_out=out["all"].data_ptr(), d_grad=grad["all"].data_ptr(), d_grad_depth=d_gdepth.data_ptr(), **dims)

    def run_none():
        gsrt.frame_loss(ctx, rgba.data_ptr(), target.data_ptr(), lam=lam, d_out=out["none"].data_ptr(),
                        d_grad=grad["none"].data_ptr(), **dims)

    def run_image_loss():
        gsrt.image_loss(ctx, rgba.data_ptr(), target.data_ptr(), lam, d_out=out["image_loss"].data_ptr(),
                        d_grad=grad["image_loss"].data_ptr(), **dims)

    variants = [("all", run_all), ("none", run_none), ("image_loss", run_image_loss)]
    for _ in range(10):
        for _, fn in variants:
            fn()
    ctx.synchronize()
    torch.cuda.synchronize()
    same = (torch.equal(out["none"][:4].view(torch.int32), out["image_loss"][:4].view(torch.int32)) and
            torch.equal(grad["none"].view(torch.int32), grad["image_loss"].view(torch.int32)))
    if not same:
        sys.exit("frame_loss_cost: the call with no option does not have gsrt_image_loss's bits")
    scalars = {k: [float(v) for v in out[k].cpu()] for k in out}

    def timed(fn):
        ctx.synchronize()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(lib_stream)
        for _ in range(a.calls):
            fn()
        e1.record(lib_stream)
        ctx.synchronize()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    ms = {k: [] for k, _ in variants}
    for r in range(a.rounds):
        for k, fn in variants[r % 3:] + variants[:r % 3]:
            ms[k].append(timed(fn))
    res = dict(width=W, height=H, lam=lam, rounds=a.rounds, calls=a.calls, none_has_image_loss_bits=same, scalars=scalars)
    for k, v in ms.items():
        res[k + "_ms"] = dict(median=float(np.median(v)), min=min(v), max=max(v))
    ref = res["image_loss_ms"]
    res["image_loss_spread"] = (ref["max"] - ref["min"]) / ref["median"]
    res["none_over_image_loss"] = res["none_ms"]["median"] / ref["median"]
    res["all_over_image_loss"] = res["all_ms"]["median"] / ref["median"]
    # the bytes a call must move at least, per pixel: rgba and the target read by both passes, nine planes written and
    # read, the gradient written; with everything on, mask, depth and target depth read by both passes and grad_depth
    px = W * H
    plain, added = 4 * (2 * (4 + 3) + 2 * 9 + 4), 4 * (2 * 3 + 1)
    res["min_bytes"] = dict(image_loss=px * plain, all=px * (plain + added), ratio=(plain + added) / plain)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
