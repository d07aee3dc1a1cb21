"""What a splat gradient frame (GSRT_FLAG_SPLAT_GRAD) and the projection's backward refuse, and in which words: through the
host hook gsrt_debug_frame_refusal_kind (no device) and through the entry points (gpu), after which the context renders as
before. The older hook, gsrt_debug_frame_refusal, keeps its answers: tests/test_frame_refusal_host.py holds it to the golden."""
import ctypes

import numpy as np
import pytest

import gsrt
from test_frame_refusal_host import frame_refusal

SPLAT = 4  # the hook's caller number of gsrt_render_splat_grad
FLAG = "GSRT_FLAG_SPLAT_GRAD"


def refusal_kind(mode, caller=0, samples=1, bvh_built=1, ntri=0, features=0, sh=0):
    msg = ctypes.create_string_buffer(256)
    s = gsrt.lib.gsrt_debug_frame_refusal_kind(mode, caller, samples, bvh_built, ntri, features, sh, msg, len(msg))
    return s, msg.value.decode()


# ------------------------------------------------------------------------------------------------ host
def test_flag_and_exports():
    assert gsrt.FLAG_SPLAT_GRAD == 0x20000
    assert {"gsrt_render_splat_grad", "gsrt_render_splat_grad_async", "gsrt_splat_grad_to_model",
            "gsrt_splat_grad_to_model_async", "gsrt_debug_frame_refusal_kind"} <= set(gsrt.EXPORTS)


def test_hook_refusals():
    M = gsrt.MODE_COR | gsrt.FLAG_SPLAT_GRAD
    assert refusal_kind(M, SPLAT) == (gsrt.OK, "")
    assert refusal_kind(M, SPLAT, sh=1, features=1) == (gsrt.OK, "")
    # the flag through any other entry point
    for caller in (0, 1, 2, 3):
        assert refusal_kind(M, caller) == (gsrt.E_ARG, FLAG + ": only through gsrt_render_splat_grad (the gradient image goes there)")
    assert refusal_kind(gsrt.MODE_REF | gsrt.FLAG_SPLAT_GRAD, SPLAT) == (gsrt.E_ARG, FLAG + ": COR frames only")
    assert refusal_kind(M | gsrt.FLAG_LUT, SPLAT) == (gsrt.E_ARG, FLAG + ": not with GSRT_FLAG_LUT")
    assert refusal_kind(M | gsrt.FLAG_STATS, SPLAT) == (gsrt.E_ARG, FLAG + ": not with GSRT_FLAG_STATS")
    assert refusal_kind(M | gsrt.FLAG_STATS | gsrt.FLAG_LUT, SPLAT) == (gsrt.E_ARG, FLAG + ": not with GSRT_FLAG_STATS")
    assert refusal_kind(M | gsrt.FLAG_OUT_DUMP8, SPLAT) == (gsrt.E_ARG, FLAG + ": not with GSRT_FLAG_OUT_DUMP8")
    for bit, name in ((gsrt.FLAG_DEPTH, "DEPTH"), (gsrt.FLAG_FEATURES, "FEATURES"), (gsrt.FLAG_FEATURE_GRAD, "FEATURE_GRAD"),
                      (gsrt.FLAG_SH_GRAD, "SH_GRAD"), (gsrt.FLAG_OPACITY_GRAD, "OPACITY_GRAD")):
        assert refusal_kind(M | bit, SPLAT, features=1, sh=1) == (gsrt.E_ARG, FLAG + ": not with GSRT_FLAG_" + name)
    assert refusal_kind(M, SPLAT, ntri=12) == (gsrt.E_ARG, FLAG + ": not for a scene with a triangle mesh")
    assert refusal_kind(M, SPLAT, samples=0) == (gsrt.E_ARG, "samples == 0")
    assert refusal_kind(M, SPLAT, bvh_built=0) == (gsrt.E_STATE, "render before gsrt_build_bvh")
    # 0x10000 stays no flag, with and without the new one
    assert refusal_kind(gsrt.MODE_COR | 0x10000, 0) == (gsrt.E_ARG, "bad mode")
    assert refusal_kind(M | 0x10000, SPLAT) == (gsrt.E_ARG, "bad mode")
    assert refusal_kind(M | 0x40000, SPLAT) == (gsrt.E_ARG, "bad mode")
    assert gsrt.lib.gsrt_debug_frame_refusal_kind(gsrt.MODE_COR, 5, 1, 1, 0, 0, 0, None, 0) == gsrt.E_ARG  # no such caller


def test_older_hook_keeps_its_callers_and_answers():
    """caller 4 stays GSRT_E_ARG there; callers 0..3 answer alike through both hooks, the new bit included"""
    assert gsrt.lib.gsrt_debug_frame_refusal(gsrt.MODE_COR | gsrt.FLAG_SPLAT_GRAD, SPLAT, 1, 1, 0, 0, 0, None, 0) == gsrt.E_ARG
    flags = (0, gsrt.FLAG_LUT, gsrt.FLAG_STATS, gsrt.FLAG_DEPTH, gsrt.FLAG_FEATURES, gsrt.FLAG_FEATURE_GRAD, gsrt.FLAG_SH_GRAD,
             gsrt.FLAG_OPACITY_GRAD, gsrt.FLAG_SPLAT_GRAD, 0x10000, gsrt.FLAG_OPACITY_GRAD | gsrt.FLAG_LUT)
    for low in (gsrt.MODE_REF, gsrt.MODE_COR, 2):
        for f in flags:
            for caller in (0, 1, 2, 3):
                for sh in (0, 1):
                    args = (low | f, caller, 1, 1, 0, 1, sh)
                    assert frame_refusal(*args) == refusal_kind(*args), args
    # a gradient frame of an earlier kind is not refused for the LUT
    assert refusal_kind(gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD | gsrt.FLAG_LUT, 3) == (gsrt.OK, "")


# ------------------------------------------------------------------------------------------------ gpu
W = H = 16
N = 100


def _scene(ctx, mesh=False, sh=True):
    c, r, s, o, table = gsrt.synth_cloud(gsrt.SYNTH_COR, N, 9, True)
    sc = gsrt.Scene.from_model(ctx, c, r, s, np.minimum(o, np.float32(0.9)), table if sh else None)
    if mesh:
        sc.add_mesh(*gsrt.sphere_mesh((0.0, 0.0, -3.0), 0.5))
    return sc


def _last(ctx):
    return gsrt.lib.gsrt_last_error(ctx.handle).decode()


@pytest.mark.gpu
def test_entry_points_refuse(ctx):
    import torch

    L, P = gsrt.lib, ctypes.c_void_p
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 1, 16)
    u = gsrt._p(ubo)
    G, rows = np.ones((H, W, 4), np.float32), np.zeros((N, 8), np.float32)
    gc, gv = np.zeros((N, 3), np.float32), np.zeros((N, 6), np.float32)
    d_G, d_rows = torch.from_numpy(G).to("cuda:0"), torch.zeros((N, 8), dtype=torch.float32, device="cuda:0")
    d_c, d_v = torch.zeros((N, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((N, 6), dtype=torch.float32, device="cuda:0")
    p = gsrt._p
    sc = _scene(ctx)
    try:
        h = sc.handle
        # before the BVH is built
        assert L.gsrt_render_splat_grad(h, u, gsrt.MODE_COR, 0, p(G), p(rows), 0) == gsrt.E_STATE
        assert L.gsrt_splat_grad_to_model(h, u, p(rows), p(gc), p(gv), 0) == gsrt.E_STATE and "gsrt_build_bvh" in _last(ctx)
        sc.build_bvh()
        before = sc.render(ubo)[0].tobytes()

        def refused(status, want_status, *words):
            assert status == want_status, (status, _last(ctx))
            for w in words:
                assert w in _last(ctx), (w, _last(ctx))
            assert sc.render(ubo)[0].tobytes() == before

        # the flag through gsrt_render and the other whole-frame entry points
        rgba = np.zeros((H, W, 4), np.float32)
        refused(L.gsrt_render(h, u, gsrt.MODE_COR | gsrt.FLAG_SPLAT_GRAD, 0, p(rgba), None), gsrt.E_ARG, FLAG, "only through")
        refused(L.gsrt_render_async(h, u, gsrt.MODE_COR | gsrt.FLAG_SPLAT_GRAD, 0, None, None), gsrt.E_ARG, FLAG)
        t1 = np.zeros(N, np.float32)
        refused(L.gsrt_render_opacity_grad(h, u, gsrt.MODE_COR | gsrt.FLAG_SPLAT_GRAD, 0, p(G), p(t1), 0), gsrt.E_ARG, FLAG)
        # LUT, REF, STATS and the other frame flags through the entry point itself, blocking and async
        for mode, word in ((gsrt.MODE_COR | gsrt.FLAG_LUT, "not with GSRT_FLAG_LUT"), (gsrt.MODE_REF, "COR frames only"),
                           (gsrt.MODE_COR | gsrt.FLAG_STATS, "not with GSRT_FLAG_STATS"),
                           (gsrt.MODE_COR | gsrt.FLAG_OUT_DUMP8, "not with GSRT_FLAG_OUT_DUMP8"),
                           (gsrt.MODE_COR | gsrt.FLAG_DEPTH, "not with GSRT_FLAG_DEPTH"),
                           (gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD, "not with GSRT_FLAG_OPACITY_GRAD"),
                           (gsrt.MODE_COR | gsrt.FLAG_SH_GRAD, "not with GSRT_FLAG_SH_GRAD")):
            want = refusal_kind(mode | gsrt.FLAG_SPLAT_GRAD, SPLAT, sh=1)
            assert want == (gsrt.E_ARG, FLAG + ": " + word)
            refused(L.gsrt_render_splat_grad(h, u, mode, 0, p(G), p(rows), 0), gsrt.E_ARG, want[1])
            refused(L.gsrt_render_splat_grad_async(h, u, mode, 0, P(d_G.data_ptr()), P(d_rows.data_ptr()), 0), gsrt.E_ARG, want[1])
        # NULL tables
        refused(L.gsrt_render_splat_grad(h, u, gsrt.MODE_COR, 0, None, p(rows), 0), gsrt.E_ARG, FLAG, "grad_image is NULL")
        refused(L.gsrt_render_splat_grad(h, u, gsrt.MODE_COR, 0, p(G), None, 0), gsrt.E_ARG, FLAG, "grad_table is NULL")
        refused(L.gsrt_render_splat_grad_async(h, u, gsrt.MODE_COR, 0, P(d_G.data_ptr()), None, 0), gsrt.E_ARG, FLAG)
        refused(L.gsrt_splat_grad_to_model(h, u, None, p(gc), p(gv), 0), gsrt.E_ARG, "grad_splat is NULL")
        refused(L.gsrt_splat_grad_to_model(h, u, p(rows), None, p(gv), 0), gsrt.E_ARG, "grad_center is NULL")
        refused(L.gsrt_splat_grad_to_model(h, u, p(rows), p(gc), None, 0), gsrt.E_ARG, "grad_cov is NULL")
        refused(L.gsrt_splat_grad_to_model_async(h, u, P(d_rows.data_ptr()), P(d_c.data_ptr()), None, 0), gsrt.E_ARG)
        assert L.gsrt_splat_grad_to_model(None, u, p(rows), p(gc), p(gv), 0) == gsrt.E_ARG
        # a host table with accumulate
        refused(L.gsrt_render_splat_grad(h, u, gsrt.MODE_COR, 0, p(G), p(rows), 1), gsrt.E_ARG, FLAG, "accumulate")
        refused(L.gsrt_splat_grad_to_model(h, u, p(rows), p(gc), P(d_v.data_ptr()), 1), gsrt.E_ARG, "accumulate")
        refused(L.gsrt_splat_grad_to_model(h, u, p(rows), P(d_c.data_ptr()), p(gv), 1), gsrt.E_ARG, "accumulate")
        # and what is let through runs
        assert L.gsrt_render_splat_grad(h, u, gsrt.MODE_COR, 0, p(G), p(rows), 0) == gsrt.OK
        assert rows[:, :6].any() and not rows[:, 6:].any()
        assert L.gsrt_splat_grad_to_model(h, u, p(rows), p(gc), p(gv), 0) == gsrt.OK and gc.any() and gv.any()
        assert L.gsrt_splat_grad_to_model(h, u, P(d_rows.data_ptr()), P(d_c.data_ptr()), P(d_v.data_ptr()), 1) == gsrt.OK
        assert sc.render(ubo)[0].tobytes() == before
    finally:
        sc.close()


@pytest.mark.gpu
def test_a_scene_with_a_mesh_is_refused(ctx):
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 1, 16)
    u, p, L = gsrt._p(ubo), gsrt._p, gsrt.lib
    G, rows = np.ones((H, W, 4), np.float32), np.zeros((N, 8), np.float32)
    gc, gv = np.zeros((N, 3), np.float32), np.zeros((N, 6), np.float32)
    sc = _scene(ctx, mesh=True)
    try:
        sc.build_bvh()
        before = sc.render(ubo, gsrt.MODE_REF, raystate=True)[1].tobytes()
        assert L.gsrt_render_splat_grad(sc.handle, u, gsrt.MODE_COR, 0, p(G), p(rows), 0) == gsrt.E_ARG
        assert _last(ctx) == FLAG + ": not for a scene with a triangle mesh"
        assert L.gsrt_splat_grad_to_model(sc.handle, u, p(rows), p(gc), p(gv), 0) == gsrt.E_ARG
        assert "triangle mesh" in _last(ctx)
        assert sc.render(ubo, gsrt.MODE_REF, raystate=True)[1].tobytes() == before
    finally:
        sc.close()
