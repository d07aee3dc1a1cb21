"""C3-geometry frames timed by gsrt_timing (render kernel and frame), all on the in-order path and on one library: the
plain SH-3 colour frame (the baseline: its kernel is the parent's), the 16-channel feature-gradient frame
(gsrt_render_feature_grad_async) and the SH gradient frame (gsrt_render_sh_grad_async), device buffers throughout.
Medians of 40 frames, three interleaved rounds."""
import os, sys, json
os.environ["GSRT_DEBUG_SLOT_STREAMS"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3dgs-raytrace_amd")]
import numpy as np
import torch
import gsrt
with gsrt.Context(0) as ctx:
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 1_000_000, 42, True)
    n = len(o)
    W, H = 1920, 1080
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    sc.build_bvh()
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 4, 16)
    g16 = torch.rand((H, W, 16), dtype=torch.float32, device="cuda:0")
    g4 = torch.rand((H, W, 4), dtype=torch.float32, device="cuda:0")
    t16 = torch.zeros((n, 16), dtype=torch.float32, device="cuda:0")
    t48 = torch.zeros((n, 48), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def frame(kind):
        if kind == "plain_sh":
            sc.render_async(ubo, gsrt.MODE_COR)
        elif kind == "feature_grad16":
            sc.feature_grad_async(ubo, g16.data_ptr(), 16, t16.data_ptr())
        else:
            sc.sh_grad_async(ubo, g4.data_ptr(), t48.data_ptr())

    kinds = ["plain_sh", "feature_grad16", "sh_grad"]
    for _ in range(10):
        for kind in kinds:
            frame(kind)
    ctx.synchronize()
    res = {kind: [] for kind in kinds}
    for rnd in range(3):
        for kind in kinds:
            ctx.timing(40)
            for _ in range(40):
                frame(kind)
            ctx.synchronize()
            k, f = ctx.timing_read()
            res[kind].append((float(np.median(k)), float(np.median(f))))
            print(f"round {rnd} {kind}: kernel median {np.median(k):.4f} ms, frame median {np.median(f):.4f} ms ({len(k)} frames)")
    print(json.dumps({kind: {"kernel_ms": [a for a, _ in v], "frame_ms": [b for _, b in v]} for kind, v in res.items()}))
