"""C3-geometry frames timed by gsrt_timing (render kernel and frame), all on the in-order path and on one library: the
forward feature frame of 16 channels (the baseline: its kernel is the parent's) and gradient frames of 1, 4 and 16
channels (gsrt_render_feature_grad_async, device buffers). Also the frame's blended lane-hits (GSRT_FLAG_STATS), which
bound the gradient kernel's atomic traffic: one wave-instruction adds 4 C bytes per candidate some lane blended, so
the bytes lie between 4 C hits / 64 (every blend shared by a full wave) and 4 C hits (no blend shared).

With --count and a counting build (make gsrt/libgsrt_xcount.so XFLAGS=-DGSRT_GRAD_AB=2, named by GSRT_LIB_PATH) the
traffic is exact instead: a 2-channel gradient frame whose channel 0 counts the adds every row receives (one per
candidate some lane of a wave blended: 4 C bytes each) and whose channel 1 counts the atomic wave-instructions.
Other A/B builds (GSRT_GRAD_AB=1: no atomic; GSRT_GRAD_WAVES=5) are timed by the plain run through GSRT_LIB_PATH."""
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
    sc.set_features(np.random.default_rng(1).uniform(-1.0, 1.0, (n, 16)).astype(np.float32))
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 4, 16)
    sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_STATS)
    hits = ctx.last_stats()["blended"]
    g = {C: torch.rand((H, W, C), dtype=torch.float32, device="cuda:0") for C in (1, 4, 16)}
    t = {C: torch.zeros((n, C), dtype=torch.float32, device="cuda:0") for C in (1, 4, 16)}
    torch.cuda.synchronize()
    if "--count" in sys.argv:
        d_t = torch.zeros((n, 2), dtype=torch.float32, device="cuda:0")
        sc.feature_grad_async(ubo, g[4].data_ptr(), 2, d_t.data_ptr())  # the image's values are not used
        ctx.synchronize()
        cnt = d_t.cpu().numpy().astype(np.float64)
        assert cnt.max() < 2 ** 24  # exact in float32
        print(json.dumps({"blended_lane_hits": hits, "row_adds": int(cnt[:, 0].sum()), "atomic_instructions": int(cnt[:, 1].sum()),
                          "rows_touched": int((cnt[:, 0] > 0).sum()), "most_adds_to_one_row": int(cnt[:, 0].max())}))
        sys.exit(0)

    def frame(kind):
        if kind == "feat16":
            sc.render_features_async(ubo)
        else:
            C = int(kind[4:])
            sc.feature_grad_async(ubo, g[C].data_ptr(), C, t[C].data_ptr())

    kinds = ["feat16", "grad1", "grad4", "grad16"]
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
    out = {kind: {"kernel_ms": [a for a, _ in v], "frame_ms": [b for _, b in v]} for kind, v in res.items()}
    out["blended_lane_hits"] = hits
    for C in (1, 4, 16):
        ms = float(np.median(out[f"grad{C}"]["kernel_ms"]))
        out[f"grad{C}_atomic_GBps_bounds"] = [4.0 * C * hits / 64 / (ms * 1e-3) / 1e9, 4.0 * C * hits / (ms * 1e-3) / 1e9]
    print(json.dumps(out))
