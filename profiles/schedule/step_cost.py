"""Time per gsrt_trainer_step of ONE library, for comparing two builds process by process, and the statistic kernels alone.

Workload: profiles/trainer/trainer_cost.py's (the C3 cloud, 1M Gaussians, SH-3, 1920 x 1080, 1 spp, a device target rendered
from a perturbed copy). A process loads the library GSRT_LIB_PATH names (or the tree's), warms up, and times `rounds`
blocks of `iters` iterations by the wall clock (each iteration ends in the step's own host synchronisation). Run it once
per build and round, alternating the builds, and compare the ranges.

With a library that has gsrt_view_stats_add it also times, over the trainer's own splat rows of its last step (the seen
share of a real frame), gsrt_density_stats_add_async and gsrt_view_stats_add_async with and without radii: the wall clock
over `calls` enqueued calls and one synchronisation, so a figure is a call's time on a busy stream, not a profiler's.

    GSRT_LIB_PATH=old/libgsrt.so python3 profiles/schedule/step_cost.py --label parent --out FILE
    python3 profiles/schedule/step_cost.py --label this --out FILE
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before gsrt: torch's HIP runtime first, as in bench.py

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "3dgs-raytrace_amd"))

import gsrt  # noqa: E402

RATES = dict(lr_center=1.6e-4, lr_rot=1e-3, lr_scale=5e-3, lr_opacity=5e-2, lr_sh_dc=2.5e-3, lr_sh_rest=1.25e-4)
LAM = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, W, H = a.n, a.width, a.height
    ctx = gsrt.Context(0)
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, n, 42, True)
    o = np.minimum(o, np.float32(0.99))
    rng = np.random.default_rng(77)
    other = ((c + rng.normal(0, 0.002, c.shape)).astype(np.float32), r, (s * rng.uniform(0.9, 1.1, s.shape)).astype(np.float32),
             (o * rng.uniform(0.7, 1.0, o.shape)).astype(np.float32), (sh + rng.normal(0, 0.05, sh.shape)).astype(np.float32))
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 1, 16)
    sc_t = gsrt.Scene.from_model(ctx, *other)
    sc_t.build_bvh()
    t_target = torch.from_numpy(np.ascontiguousarray(sc_t.render(ubo)[0][..., :3])).to("cuda:0")
    sc_t.close()
    tr = gsrt.Trainer(ctx, (c, r, s, o, sh))
    adam = gsrt.adam_params(**RATES, sparse=True)

    def iters(k):
        for _ in range(k):
            tr.step(ubo, t_target.data_ptr(), adam, lam=LAM, target_channels=3, want_scalars=True)

    iters(5)  # warm-up: allocations, clocks
    ts = []
    for _ in range(a.rounds):
        ctx.synchronize()
        t0 = time.perf_counter()
        iters(a.iters)
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) / a.iters * 1e3)
    res = {"label": a.label, "lib": os.environ.get("GSRT_LIB_PATH", "tree"), "n": n, "width": W, "height": H,
           "iters": a.iters, "step_ms": ts}

    if hasattr(gsrt.lib, "gsrt_view_stats_add_async"):
        rows = tr.state()["grads"][2]
        scene = tr.scene()
        d_stats = torch.zeros((n, 2), dtype=torch.float32, device="cuda:0")
        d_radii = torch.zeros((n,), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()

        def timed(fn):
            fn()
            ctx.synchronize()
            out = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                ctx.synchronize()
                out.append((time.perf_counter() - t0) / a.calls * 1e6)
            return {"us": float(np.median(out)), "us_min": float(min(out)), "us_max": float(max(out))}

        res["density_stats_add"] = timed(lambda: gsrt.density_stats_add(ctx, rows, d_stats.data_ptr(), W, H, n=n, asynchronous=True))
        res["view_stats_add_no_radii"] = timed(lambda: scene.view_stats_add(ubo, rows, d_stats.data_ptr(), None, asynchronous=True))
        res["view_stats_add"] = timed(lambda: scene.view_stats_add(ubo, rows, d_stats.data_ptr(), d_radii.data_ptr(), asynchronous=True))
        res["seen"] = int((d_stats[:, 1] > 0).sum().item())
        res["radii_set"] = int((d_radii > 0).sum().item())
        res["radii_max"] = float(d_radii.max().item())
    tr.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
