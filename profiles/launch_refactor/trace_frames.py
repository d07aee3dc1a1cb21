"""Every frame kind launch_render serves, once, on one context at 256x256 with 10k Gaussians: the workload whose HIP API
and kernel traces are compared between two builds of the library (GSRT_LIB_PATH), see compare_traces.py.

  rocprofv3 --hip-trace --kernel-trace --output-format csv -d <dir> -- python3 profiles/launch_refactor/trace_frames.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "3dgs-raytrace_amd"))
import gsrt  # noqa: E402

W = H = 256
N = 10_000

with gsrt.Context(0) as ctx:
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, N, 7, True)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    mv = gsrt.lookat((0, 0, 0), (0, 0, -1))
    ubo = gsrt.camera_from_modelview(mv, 60.0, W, H, 1.0, 4, 16)
    sums = []
    for _ in range(4):  # plain COR frames (the first sizes the slots, the later ones rotate them)
        sums.append(sc.render(ubo, gsrt.MODE_COR)[0].sum())
    sums.append(sc.render(ubo, gsrt.MODE_REF, raystate=True)[1]["trans"].sum())
    sums.append(sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_STATS)[0].sum())
    sums.append(sc.render_depth(ubo)[1].sum())
    sc.set_features(np.linspace(0.0, 1.0, N * 3, dtype=np.float32).reshape(N, 3))
    sums.append(sc.render_features(ubo)[1].sum())
    sums.append(sc.feature_grad(ubo, np.ones((H, W, 3), np.float32)).sum())
    sums.append(sc.render_sharded_emulated(ubo, 4).sum())
    params, aabbs = sc.download()
    sc.update(params, aabbs)
    sums.append(sc.render(ubo, gsrt.MODE_COR)[0].sum())
    sums.append(sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_LUT)[0].sum())
    print("frames ok:", " ".join(f"{float(v):.6g}" for v in sums))
