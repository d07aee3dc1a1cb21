"""Time of the fused optimiser step (gsrt_model_step_async) against the torch code it replaces, on the same GPU in the same
process, at 1M Gaussians with SH.

  python3 profiles/model_step.py [--n 1000000 --rounds 5 --calls 50 --out FILE]

(a) fused: gsrt_model_step_async with params_out and aabbs_out (no act, no grad_raw: a loop's steady state), dense, and
    sparse with the splat rows of every second Gaussian +0 (half the model unseen).
(b) torch, what a step of the render_model loop runs between the backward's tables and the next Scene.update:
    normalise / exp / sigmoid and gsrt.autograd.model_covariance forward, their autograd backward from the same d cov3d and
    d opacity, torch.optim.Adam over the five tensors (foreach=False, fused=False: "adam_loop"; foreach=True:
    "adam_foreach"), and the (n, 12) params / (n, 6) AABB packing of _RenderModel.forward. This code is the parent
    revision's as it stands (gsrt/autograd.py's model_covariance and packing are unchanged).

Method (measuring-on-mi355x): all variants are warmed up (5 calls each), then `rounds` rounds alternate them; in a round
each runs `calls` times back to back between two device events on its own stream (the library's stream, torch's current
stream) with a device synchronise before and after: device time per call including launch gaps, as a training loop sees
it. Per variant: the median over rounds, the smallest and the largest round. The fused step's bytes are counted from the
code (gsrt_model_step.hip) and divided by its time; the share is of the 8.0 TB/s datasheet peak and of the 6.29 TB/s a
float4 copy reaches (MI355X_MICROARCH.md). No GPU: the script fails, it does not fall back."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3dgs-raytrace_amd"))
import gsrt  # noqa: E402
from gsrt.autograd import model_covariance  # noqa: E402

RATES = dict(lr_center=1.6e-4, lr_rot=1e-3, lr_scale=5e-3, lr_opacity=5e-2, lr_sh_dc=2.5e-3, lr_sh_rest=2.5e-3)


def step_bytes(n, seen):
    """HBM bytes of one fused step from the code: per stepped Gaussian raw, m, v (59 words each) in and out and the
    gradient tables in (centre 3, cov 6, splat 8, sh 48 words); per Gaussian 72 B of scene arrays out; sparse (seen < n)
    the row kernel reads the splat row again, and an unseen Gaussian costs its 11 raw words and its splat row"""
    stepped = seen * (4 * (3 * 59 + 65) + 4 * 3 * 59)
    unseen = (n - seen) * (4 * 11 + 32)
    again = 32 * n if seen < n else 0
    return stepped + unseen + again + 72 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("model_step: no GPU")
    n, dev = a.n, torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(3)
    rnd = lambda *shape: torch.randn(shape, generator=g)  # noqa: E731
    raw0 = [rnd(n, 3), rnd(n, 4), -3.0 + 0.3 * rnd(n, 3), rnd(n), 0.3 * rnd(n, 48)]
    grads0 = [1e-3 * rnd(n, 3), 1e-3 * rnd(n, 6), 1e-3 * rnd(n, 8), 1e-3 * rnd(n, 48)]
    half = grads0[2].clone()
    half[1::2, :6] = 0.0
    to = lambda t: t.to(dev).contiguous()  # noqa: E731
    ctx = gsrt.Context(0)
    lib_stream = torch.cuda.ExternalStream(ctx.stream, device=dev)

    # (a) fused
    raw, m, v = [to(t) for t in raw0], [torch.zeros_like(to(t)) for t in raw0], [torch.zeros_like(to(t)) for t in raw0]
    d_c, d_cov, d_rows, d_sh = (to(t) for t in grads0)
    d_half = to(half)
    params, aabbs = torch.empty((n, 12), device=dev), torch.empty((n, 6), device=dev)
    ptrs = lambda ts: [t.data_ptr() for t in ts] + [0]  # noqa: E731
    count = {"t": 0}

    def fused(rows, sparse):
        count["t"] += 1
        gsrt.model_step(ctx, ptrs(raw), ptrs(m), ptrs(v), [d_c.data_ptr(), d_cov.data_ptr(), rows.data_ptr(), d_sh.data_ptr(), 0],
                        gsrt.adam_params(**RATES, step=count["t"], sparse=sparse), n=n, params_out=params.data_ptr(),
                        aabbs_out=aabbs.data_ptr(), asynchronous=True)

    # (b) torch
    def torch_variant(foreach):
        p = [to(t).requires_grad_(True) for t in raw0]
        opt = torch.optim.Adam([dict(params=[p[0]], lr=RATES["lr_center"]), dict(params=[p[1]], lr=RATES["lr_rot"]),
                                dict(params=[p[2]], lr=RATES["lr_scale"]), dict(params=[p[3]], lr=RATES["lr_opacity"]),
                                dict(params=[p[4]], lr=RATES["lr_sh_dc"])], betas=(0.9, 0.999), eps=1e-15,
                               foreach=foreach, fused=False)
        d_op = d_rows[:, 5].contiguous()

        def step():
            opt.zero_grad(set_to_none=True)
            q, s, o = torch.nn.functional.normalize(p[1], dim=1), torch.exp(p[2]), torch.sigmoid(p[3])
            cov = model_covariance(q, s)
            torch.autograd.backward([cov, o], [d_cov, d_op])
            p[0].grad, p[4].grad = d_c, d_sh
            opt.step()
            with torch.no_grad():
                q, s, o = torch.nn.functional.normalize(p[1], dim=1), torch.exp(p[2]), torch.sigmoid(p[3])
                cov = model_covariance(q, s)
                out = torch.zeros((n, 12), dtype=torch.float32, device=dev)
                out[:, 0:3], out[:, 3], out[:, 4:10] = p[0], o, cov
                rad = 3.0 * s.max(dim=1, keepdim=True).values
                return out, torch.cat([p[0] - rad, p[0] + rad], 1)
        return step

    variants = {"fused_dense": (lambda: fused(d_rows, False), lib_stream),
                "fused_sparse_half": (lambda: fused(d_half, True), lib_stream),
                "torch_adam_loop": (torch_variant(False), torch.cuda.current_stream(dev)),
                "torch_adam_foreach": (torch_variant(True), torch.cuda.current_stream(dev))}

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

    for fn, _ in variants.values():
        for _ in range(5):
            fn()
    ctx.synchronize()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, (fn, stream) in variants.items():
            ms[k].append(timed(fn, stream))
    res = dict(n=n, rounds=a.rounds, calls=a.calls)
    for k, t in ms.items():
        res[k + "_ms"] = dict(median=float(np.median(t)), min=min(t), max=max(t))
    for k, seen in (("fused_dense", n), ("fused_sparse_half", n - n // 2)):
        b = step_bytes(n, seen)
        tbs = b / (res[k + "_ms"]["median"] * 1e-3) / 1e12
        res[k + "_bytes"] = b
        res[k + "_TBps"] = tbs
        res[k + "_share_of_8.0"] = tbs / 8.0
        res[k + "_share_of_6.29_copy"] = tbs / 6.29
    for k in ("torch_adam_loop", "torch_adam_foreach"):
        res[k + "_over_fused_dense"] = res[k + "_ms"]["median"] / res["fused_dense_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
