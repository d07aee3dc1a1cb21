"""The 20k synthetic cloud at 64x48 timed by gsrt_timing (render kernel and frame), all on the in-order path: the plain
colour frame and the opacity gradient frame (gsrt_render_opacity_grad_async) of the same scene and camera, without and
with SH-3 rows, at 3 spp (three passes) and 4 spp (samples in the wave), device buffers throughout. Medians of 40
frames, three interleaved rounds. --plain-only: the plain frames alone (a library named by GSRT_LIB_PATH that predates
the gradient frame, i.e. the parent's)."""
import os, sys, json
os.environ["GSRT_DEBUG_SLOT_STREAMS"] = "0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "3dgs-raytrace_amd")]
import numpy as np
import torch
import gsrt
plain_only = "--plain-only" in sys.argv
with gsrt.Context(0) as ctx:
    W, H = 64, 48
    res = {}
    for with_sh in (False, True):
        c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 20000, 7, with_sh)
        n = len(o)
        sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh if with_sh else None)
        sc.build_bvh()
        g4 = torch.rand((H, W, 4), dtype=torch.float32, device="cuda:0")
        t = torch.zeros((n,), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for spp in (3, 4):
            ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, spp, 16)

            def frame(kind):
                if kind == "plain":
                    sc.render_async(ubo, gsrt.MODE_COR)
                else:
                    sc.opacity_grad_async(ubo, g4.data_ptr(), t.data_ptr())

            kinds = ["plain"] if plain_only else ["plain", "opacity_grad"]
            for _ in range(10):
                for kind in kinds:
                    frame(kind)
            ctx.synchronize()
            for rnd in range(3):
                for kind in kinds:
                    ctx.timing(40)
                    for _ in range(40):
                        frame(kind)
                    ctx.synchronize()
                    k, f = ctx.timing_read()
                    res.setdefault(f"{kind} sh={int(with_sh)} spp={spp}", []).append((float(np.median(k)), float(np.median(f))))
        sc.close()
    for key, v in res.items():
        print(f"{key}: kernel medians {[round(a, 4) for a, _ in v]} ms, frame medians {[round(b, 4) for _, b in v]} ms")
    print(json.dumps({key: {"kernel_ms": [a for a, _ in v], "frame_ms": [b for _, b in v]} for key, v in res.items()}))
