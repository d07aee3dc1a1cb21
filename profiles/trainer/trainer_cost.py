"""Time per training iteration: gsrt.Trainer.step beside the composed loop it replaces (the torch-free loop of
tests/test_model_step_gpu.py::test_end_to_end, torch tensors as its memory), interleaved in one process.

Workload: the C3 cloud (gsrt_synth_cloud, 1M Gaussians, SH-3) at 1920 x 1080, 1 spp, against a target rendered from a
perturbed copy. Rounds alternate the two sides in rotating order; a side's figure for a round is wall-clock time over
`iters` iterations (each ends with the host synchronisation its sequence needs, so the wall clock is the iteration).
Also: gsrt_normal_noise (6M floats) and gsrt_model_remap (1M rows with SH, the origin of a real densify) as GB/s of the
bytes they must move.

    python3 profiles/trainer/trainer_cost.py [--n 1000000] [--rounds 5] [--iters 20] [--out FILE]
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from gsrt.autograd import model_step

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
    target = np.ascontiguousarray(sc_t.render(ubo)[0][..., :3])
    sc_t.close()
    dev = "cuda:0"
    t_target = torch.from_numpy(target).to(dev)

    # the trainer
    tr = gsrt.Trainer(ctx, (c, r, s, o, sh))
    adam = gsrt.adam_params(**RATES, sparse=True)

    def trainer_iters(k):
        for _ in range(k):
            tr.step(ubo, t_target.data_ptr(), adam, lam=LAM, target_channels=3, want_scalars=True)

    # the composed loop
    raw_np = gsrt.model_deactivate(ctx, (c, r, s, o, sh))
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    t_raw = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in raw_np[:5]] + [None]
    t_m = [torch.zeros_like(t) for t in t_raw[:5]] + [None]
    t_v = [torch.zeros_like(t) for t in t_raw[:5]] + [None]
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    t_rgba, t_gimg, t_rows, t_c, t_cov, t_sh, t_out = new(H, W, 4), new(H, W, 4), new(n, 8), new(n, 3), new(n, 6), new(n, 48), new(4)
    torch.cuda.synchronize()
    state = {"t": 0}

    def composed_iters(k):
        for _ in range(k):
            state["t"] += 1
            sc.render_async(ubo, d_rgba=t_rgba.data_ptr())
            gsrt.image_loss(ctx, t_rgba.data_ptr(), t_target.data_ptr(), LAM, width=W, height=H, target_channels=3,
                            d_out=t_out.data_ptr(), d_grad=t_gimg.data_ptr(), asynchronous=True)
            sc.splat_grad_async(ubo, t_gimg.data_ptr(), t_rows.data_ptr())
            sc.model_grad_async(ubo, t_rows.data_ptr(), t_c.data_ptr(), t_cov.data_ptr())
            sc.sh_grad_async(ubo, t_gimg.data_ptr(), t_sh.data_ptr())
            out = model_step(ctx, t_raw, t_m, t_v, (t_c, t_cov, t_rows, t_sh), gsrt.adam_params(**RATES, step=state["t"], sparse=True))
            float(t_out[0].item())
            sc.update(params=out["params"].data_ptr(), aabbs=out["aabbs"].data_ptr())
            sc.refit_bvh()
            sc.set_sh(t_raw[4].data_ptr())
            ctx.synchronize()

    sides = {"trainer": trainer_iters, "composed": composed_iters}
    for f in sides.values():  # warm-up: allocations, clocks
        f(5)
    times = {k: [] for k in sides}
    names = list(sides)
    for rnd in range(a.rounds):
        for name in names[rnd % 2:] + names[:rnd % 2]:
            ctx.synchronize()
            t0 = time.perf_counter()
            sides[name](a.iters)
            ctx.synchronize()
            times[name].append((time.perf_counter() - t0) / a.iters * 1e3)
    res = {"n": n, "width": W, "height": H, "rounds": a.rounds, "iters": a.iters}
    for name, ts in times.items():
        res[name + "_ms"] = {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts)), "rounds": ts}
    sc.close()

    # the two new kernels, against the bytes they must move
    d_noise = new(6 * n)
    torch.cuda.synchronize()

    def timed(fn, calls=50):
        fn()
        ctx.synchronize()
        best = []
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            ctx.synchronize()
            best.append((time.perf_counter() - t0) / calls)
        return float(np.median(best)), float(min(best)), float(max(best))

    med, lo, hi = timed(lambda: gsrt.normal_noise(ctx, 6 * n, 1, 0, d_out=d_noise.data_ptr(), asynchronous=True))
    res["normal_noise"] = {"floats": 6 * n, "ms": med * 1e3, "ms_min": lo * 1e3, "ms_max": hi * 1e3, "GBps": 24.0 * n / med / 1e9}
    stats = np.stack([rng.uniform(0, 2, n), np.ones(n)], 1).astype(np.float32)
    P = gsrt.densify_params(1.0, float(np.median(s.max(1))), 0.05)
    noise = gsrt.normal_noise(ctx, 6 * n, 1, 0).reshape(n, 2, 3)
    origin = gsrt.densify(ctx, c, r, s, o, None, stats, noise, P)[6]
    k = origin.size
    d_org = torch.from_numpy(origin).to(dev)
    widths = (3, 4, 3, 1, 48)
    d_in = [new(n * w).normal_() for w in widths]
    d_out = [new(k * w) for w in widths]
    torch.cuda.synchronize()
    med, lo, hi = timed(lambda: gsrt.model_remap(ctx, d_org.data_ptr(), tuple(t.data_ptr() for t in d_in) + (0,), n_out=k,
                                                 out=tuple(t.data_ptr() for t in d_out) + (0,), asynchronous=True))
    kept = int((origin >= 0).sum())
    moved = 4 * k + 236 * k + 236 * kept  # origin, every output row written, the kept rows read
    res["model_remap"] = {"n_in": n, "n_out": k, "kept": kept, "ms": med * 1e3, "ms_min": lo * 1e3, "ms_max": hi * 1e3,
                          "bytes": moved, "GBps": moved / med / 1e9}
    tr.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
