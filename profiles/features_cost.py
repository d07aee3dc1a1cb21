"""C3-geometry frames timed by gsrt_timing (kernel and frame), all on the in-order path and on one library: the plain
SH-3 frame, the plain frame of the same geometry without SH rows, and feature frames of 16 and of 1 channel."""
import os, sys, json
os.environ["GSRT_DEBUG_SLOT_STREAMS"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3dgs-raytrace_amd")]
import numpy as np
import torch  # noqa: F401
import gsrt
with gsrt.Context(0) as ctx:
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 1_000_000, 42, True)
    table = np.random.default_rng(1).uniform(-1.0, 1.0, (len(o), 16)).astype(np.float32)
    scenes = {"sh": gsrt.Scene.from_model(ctx, c, r, s, o, sh), "nosh": gsrt.Scene.from_model(ctx, c, r, s, o),
              "feat16": gsrt.Scene.from_model(ctx, c, r, s, o, sh), "feat1": gsrt.Scene.from_model(ctx, c, r, s, o, sh)}
    for sc in scenes.values():
        sc.build_bvh()
    scenes["feat16"].set_features(table)
    scenes["feat1"].set_features(table[:, :1])
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, 1920, 1080, 1.0, 4, 16)

    def frame(kind):
        if kind.startswith("feat"):
            scenes[kind].render_features_async(ubo)
        else:
            scenes[kind].render_async(ubo, gsrt.MODE_COR)

    for _ in range(20):
        for kind in scenes:
            frame(kind)
    ctx.synchronize()
    res = {kind: [] for kind in scenes}
    for rnd in range(3):
        for kind in scenes:
            ctx.timing(40)
            for _ in range(40):
                frame(kind)
            ctx.synchronize()
            k, f = ctx.timing_read()
            res[kind].append((float(np.median(k)), float(np.median(f))))
            print(f"round {rnd} {kind}: kernel median {np.median(k):.4f} ms, frame median {np.median(f):.4f} ms ({len(k)} frames)")
    out = {kind: {"kernel_ms": [a for a, _ in v], "frame_ms": [b for _, b in v]} for kind, v in res.items()}
    print(json.dumps(out))
