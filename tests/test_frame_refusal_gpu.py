"""The whole-frame entry points refuse what gsrt_debug_frame_refusal says they refuse, in its words (the hook itself is held
to the hand-written blocks it replaced by test_frame_refusal_host.py), run what it lets through, and a refused call leaves
the next frame as it was."""
import ctypes

import numpy as np
import pytest

import gsrt
from test_frame_refusal_host import frame_refusal

pytestmark = pytest.mark.gpu

W = H = 16
N = 100
FLAGS = (gsrt.FLAG_LUT, gsrt.FLAG_STATS, gsrt.FLAG_OUT_DUMP8, gsrt.FLAG_DEPTH, gsrt.FLAG_FEATURES, gsrt.FLAG_FEATURE_GRAD,
         gsrt.FLAG_SH_GRAD, gsrt.FLAG_OPACITY_GRAD)
MODES = [gsrt.MODE_COR | f for f in FLAGS] + [gsrt.MODE_REF]


def entry_points(sc, ubo):
    """name -> (caller kind of the hook, the flag the entry point sets itself, mode -> status); the blocking calls with host
    arrays, the async ones with device arrays (a gradient call's) or none"""
    import torch

    L, P, u = gsrt.lib, ctypes.c_void_p, gsrt._p(ubo)
    rgba, plane, feat = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W, 16), np.float32)
    g3, g4 = np.ones((H, W, 3), np.float32), np.ones((H, W, 4), np.float32)
    t3, t48, t1 = np.zeros((N, 3), np.float32), np.zeros((N, 48), np.float32), np.zeros(N, np.float32)
    dev = {k: torch.from_numpy(a).to("cuda:0") for k, a in dict(g3=g3, g4=g4, t3=t3, t48=t48, t1=t1).items()}
    d = {k: P(t.data_ptr()) for k, t in dev.items()}
    h, p = sc.handle, gsrt._p
    return dev, {
        "render": (0, 0, lambda m: L.gsrt_render(h, u, m, 0, p(rgba), None)),
        "render_async": (0, 0, lambda m: L.gsrt_render_async(h, u, m, 0, None, None)),
        "render_depth": (0, gsrt.FLAG_DEPTH, lambda m: L.gsrt_render_depth(h, u, m, 0, p(rgba), p(plane))),
        "render_depth_async": (0, gsrt.FLAG_DEPTH, lambda m: L.gsrt_render_depth_async(h, u, m, 0, None, None)),
        "render_features": (0, gsrt.FLAG_FEATURES, lambda m: L.gsrt_render_features(h, u, m, 0, p(rgba), p(feat))),
        "render_features_async": (0, gsrt.FLAG_FEATURES, lambda m: L.gsrt_render_features_async(h, u, m, 0, None, None)),
        "feature_grad": (1, gsrt.FLAG_FEATURE_GRAD, lambda m: L.gsrt_render_feature_grad(h, u, m, 0, p(g3), 3, p(t3), 0)),
        "feature_grad_async": (1, gsrt.FLAG_FEATURE_GRAD,
                               lambda m: L.gsrt_render_feature_grad_async(h, u, m, 0, d["g3"], 3, d["t3"], 0)),
        "sh_grad": (2, gsrt.FLAG_SH_GRAD, lambda m: L.gsrt_render_sh_grad(h, u, m, 0, p(g4), p(t48), 0)),
        "sh_grad_async": (2, gsrt.FLAG_SH_GRAD, lambda m: L.gsrt_render_sh_grad_async(h, u, m, 0, d["g4"], d["t48"], 0)),
        "opacity_grad": (3, gsrt.FLAG_OPACITY_GRAD, lambda m: L.gsrt_render_opacity_grad(h, u, m, 0, p(g4), p(t1), 0)),
        "opacity_grad_async": (3, gsrt.FLAG_OPACITY_GRAD,
                               lambda m: L.gsrt_render_opacity_grad_async(h, u, m, 0, d["g4"], d["t1"], 0)),
    }


@pytest.mark.parametrize("kind", ["sh and features", "bare", "mesh"])
def test_entry_points_refuse_what_the_hook_refuses(ctx, kind):
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, N, 9, True)
    sc = gsrt.Scene.from_model(ctx, c, r, s, np.minimum(o, np.float32(0.9)), None if kind == "bare" else sh)
    if kind != "bare":
        sc.set_features(np.linspace(-1.0, 1.0, N * 3, dtype=np.float32).reshape(N, 3))
    if kind == "mesh":
        sc.add_mesh(*gsrt.sphere_mesh((0.0, 0.0, -3.0), 0.5))
    sc.build_bvh()
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 1, 16)
    facts = dict(ntri=sc.mesh_triangles, features=int(sc.features() > 0), sh=int(kind != "bare"))
    assert facts == dict(ntri=1024 if kind == "mesh" else 0, features=int(kind != "bare"), sh=facts["sh"])

    def frame():  # what a refused call must leave alone; a scene with a mesh renders in REF mode only (its image: the ray states)
        if kind == "mesh":
            return sc.render(ubo, gsrt.MODE_REF, raystate=True)[1].tobytes()
        return sc.render(ubo)[0].tobytes()

    before = frame()
    keep, calls = entry_points(sc, ubo)
    assert len(calls) == 12  # six pairs: gsrt_render, depth, features and the three gradient calls, each with its async form
    refused = passed = 0
    for name, (caller, own, call) in calls.items():
        for mode in MODES:
            want = frame_refusal(mode | own, caller, 1, 1, **facts)
            status = call(mode)
            if want[0] == gsrt.OK:
                assert status == gsrt.OK, (name, hex(mode), status, gsrt.lib.gsrt_last_error(ctx.handle).decode())
                ctx.synchronize()
                passed += 1
            else:
                assert (status, gsrt.lib.gsrt_last_error(ctx.handle).decode()) == want, (name, hex(mode))
                assert frame() == before, (name, hex(mode))
                refused += 1
    assert refused and passed and refused + passed == 12 * 9
    assert frame() == before
    del keep
    sc.close()
