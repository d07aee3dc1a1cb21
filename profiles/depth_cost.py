"""C3 frame with and without FLAG_DEPTH, timed by gsrt_timing (kernel and frame), both on the in-order path."""
import os, sys, json
os.environ["GSRT_DEBUG_SLOT_STREAMS"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3dgs-raytrace_amd")]
import numpy as np
import torch  # noqa: F401
import gsrt
with gsrt.Context(0) as ctx:
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 1_000_000, 42, True)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, 1920, 1080, 1.0, 4, 16)
    for _ in range(20):
        sc.render_async(ubo, gsrt.MODE_COR)
        sc.render_depth_async(ubo)
    ctx.synchronize()
    res = {"plain": [], "depth": []}
    for rnd in range(3):
        for kind in ("plain", "depth"):
            ctx.timing(40)
            for _ in range(40):
                if kind == "plain":
                    sc.render_async(ubo, gsrt.MODE_COR)
                else:
                    sc.render_depth_async(ubo)
            ctx.synchronize()
            k, f = ctx.timing_read()
            res[kind].append((float(np.median(k)), float(np.median(f))))
            print(f"round {rnd} {kind}: kernel median {np.median(k):.4f} ms, frame median {np.median(f):.4f} ms ({len(k)} frames)")
    out = {kind: {"kernel_ms": [a for a, _ in v], "frame_ms": [b for _, b in v]} for kind, v in res.items()}
    print(json.dumps(out))
