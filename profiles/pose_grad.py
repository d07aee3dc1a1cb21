"""Time of the camera's gradient (gsrt_pose_grad_async) against the projection's backward (gsrt_splat_grad_to_model_async) at
the same n, on the same GPU in the same process, at 1M Gaussians.

  python3 profiles/pose_grad.py [--n 1000000 --rounds 7 --calls 50 --out FILE]

The chain call is the yardstick: it reads the same 80 B per Gaussian (48 B of parameters, 32 B of the splat row) and also
writes 36 B (centre 3 and cov3d 6 floats). It is the parent revision's code as it stands, measured here, never assumed.
The pose call reads the 80 B and writes one partial of 128 B per 2048 Gaussians, then one workgroup sums the partials.

Method (measuring-on-mi355x): both variants, plain and depth form, are warmed up (10 calls each), then `rounds` rounds
alternate them; in a round each runs `calls` times back to back on the library's stream between two device events, with a
device synchronise before and after: device time per call including launch gaps, as a training loop sees it. Per variant:
the median over rounds, the smallest and the largest round, and the bytes per second its counted traffic comes to, as a share
of the 6.29 TB/s a float4 copy reaches (MI355X_MICROARCH.md). No GPU: the script fails, it does not fall back."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "3dgs-raytrace_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gsrt  # noqa: E402
import pose_cases as PC  # noqa: E402  (the tests' synthetic model: centres in a frustum, a sixth behind the camera)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pose_grad: no GPU")
    n = a.n
    chunk, lanes = gsrt.pose_grad_layout()
    ubo = PC.camera()
    params, aabbs, rows, _ = PC.synthetic(n, 5)
    res = {}
    with gsrt.Context(0) as ctx:
        sc = gsrt.Scene.from_params(ctx, params, aabbs)
        sc.build_bvh()
        d_rows = torch.from_numpy(rows).to("cuda:0")
        d_c = torch.empty((n, 3), dtype=torch.float32, device="cuda:0")
        d_v = torch.empty((n, 6), dtype=torch.float32, device="cuda:0")
        d_out = torch.empty((16,), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        stream = torch.cuda.ExternalStream(ctx.stream)
        variants = {
            "chain": lambda: sc.model_grad_async(ubo, d_rows.data_ptr(), d_c.data_ptr(), d_v.data_ptr()),
            "chain_depth": lambda: sc.model_grad_async(ubo, d_rows.data_ptr(), d_c.data_ptr(), d_v.data_ptr(), depth=True),
            "pose": lambda: sc.pose_grad_async(ubo, d_rows.data_ptr(), d_out.data_ptr()),
            "pose_depth": lambda: sc.pose_grad_async(ubo, d_rows.data_ptr(), d_out.data_ptr(), depth=True),
        }
        for fn in variants.values():
            for _ in range(10):
                fn()
        ctx.synchronize()
        times = {k: [] for k in variants}
        for _ in range(a.rounds):
            for name, fn in variants.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.calls):
                    fn()
                e1.record(stream)
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)  # us per call
        sc.close()
    chunks = (n + chunk - 1) // chunk
    traffic = {"chain": 116 * n, "chain_depth": 116 * n, "pose": 80 * n + 2 * 128 * chunks + 64,
               "pose_depth": 80 * n + 2 * 128 * chunks + 64}
    for name, t in times.items():
        med = float(np.median(t))
        res[name] = dict(us_median=round(med, 2), us_min=round(min(t), 2), us_max=round(max(t), 2), bytes=traffic[name],
                         tb_per_s=round(traffic[name] / med / 1e6, 3), share_of_copy=round(traffic[name] / med / 1e6 / 6.29, 3))
    out = dict(n=n, rounds=a.rounds, calls=a.calls, chunk=chunk, final_lanes=lanes, chunks=chunks, **res,
               pose_over_chain=round(res["pose"]["us_median"] / res["chain"]["us_median"], 3))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
