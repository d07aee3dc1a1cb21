"""What a splat-depth gradient frame (GSRT_FLAG_SPLAT_DEPTH_GRAD) and the depth chain refuse, and in which words: through
the host hook gsrt_debug_frame_refusal_any (no device) and through the entry points (gpu), after which the context renders
as before. The older hooks keep their callers and answers: gsrt_debug_frame_refusal_kind refuses caller 5 and still calls
0x40000 a bad mode (tests/test_splat_grad_refusal.py), gsrt_debug_frame_refusal is held to the golden
(tests/test_frame_refusal_host.py); the flag is therefore 0x80000 and 0x40000 stays no flag, as 0x10000 did."""
import ctypes

import numpy as np
import pytest

import gsrt
from test_frame_refusal_host import frame_refusal
from test_splat_grad_refusal import refusal_kind

DEPTH = 5  # the hook's caller number of gsrt_render_splat_depth_grad
FLAG = "GSRT_FLAG_SPLAT_DEPTH_GRAD"
ENTRY = "gsrt_render_splat_depth_grad"


def refusal_any(mode, caller=0, samples=1, bvh_built=1, ntri=0, features=0, sh=0):
    msg = ctypes.create_string_buffer(256)
    s = gsrt.lib.gsrt_debug_frame_refusal_any(mode, caller, samples, bvh_built, ntri, features, sh, msg, len(msg))
    return s, msg.value.decode()


# ------------------------------------------------------------------------------------------------ host
def test_flag_and_exports():
    assert gsrt.FLAG_SPLAT_DEPTH_GRAD == 0x80000
    assert {"gsrt_render_splat_depth_grad", "gsrt_render_splat_depth_grad_async", "gsrt_splat_depth_grad_to_model",
            "gsrt_splat_depth_grad_to_model_async", "gsrt_debug_frame_refusal_any"} <= set(gsrt.EXPORTS)
    assert gsrt.lib.gsrt_abi_version() == 2


def test_hook_refusals():
    M = gsrt.MODE_COR | gsrt.FLAG_SPLAT_DEPTH_GRAD
    assert refusal_any(M, DEPTH) == (gsrt.OK, "")
    assert refusal_any(M, DEPTH, sh=1, features=1) == (gsrt.OK, "")
    # the flag through any other entry point
    for caller in (0, 1, 2, 3, 4):
        assert refusal_any(M, caller) == (gsrt.E_ARG, FLAG + ": only through " + ENTRY + " (the gradient image goes there)")
    assert refusal_any(gsrt.MODE_REF | gsrt.FLAG_SPLAT_DEPTH_GRAD, DEPTH) == (gsrt.E_ARG, FLAG + ": COR frames only")
    assert refusal_any(M | gsrt.FLAG_LUT, DEPTH) == (gsrt.E_ARG, FLAG + ": not with GSRT_FLAG_LUT")
    assert refusal_any(M | gsrt.FLAG_STATS, DEPTH) == (gsrt.E_ARG, FLAG + ": not with GSRT_FLAG_STATS")
    assert refusal_any(M | gsrt.FLAG_STATS | gsrt.FLAG_LUT, DEPTH) == (gsrt.E_ARG, FLAG + ": not with GSRT_FLAG_STATS")
    assert refusal_any(M | gsrt.FLAG_OUT_DUMP8, DEPTH) == (gsrt.E_ARG, FLAG + ": not with GSRT_FLAG_OUT_DUMP8")
    for bit, name in ((gsrt.FLAG_DEPTH, "DEPTH"), (gsrt.FLAG_FEATURES, "FEATURES"), (gsrt.FLAG_FEATURE_GRAD, "FEATURE_GRAD"),
                      (gsrt.FLAG_SH_GRAD, "SH_GRAD"), (gsrt.FLAG_OPACITY_GRAD, "OPACITY_GRAD"),
                      (gsrt.FLAG_SPLAT_GRAD, "SPLAT_GRAD")):
        assert refusal_any(M | bit, DEPTH, features=1, sh=1) == (gsrt.E_ARG, FLAG + ": not with GSRT_FLAG_" + name)
    assert refusal_any(M, DEPTH, ntri=12) == (gsrt.E_ARG, FLAG + ": not for a scene with a triangle mesh")
    assert refusal_any(M, DEPTH, samples=0) == (gsrt.E_ARG, "samples == 0")
    assert refusal_any(M, DEPTH, bvh_built=0) == (gsrt.E_STATE, "render before gsrt_build_bvh")
    # 0x10000 and 0x40000 stay no flags, with and without the new one
    for bad in (0x10000, 0x40000):
        assert refusal_any(gsrt.MODE_COR | bad, 0) == (gsrt.E_ARG, "bad mode")
        assert refusal_any(M | bad, DEPTH) == (gsrt.E_ARG, "bad mode")
    # a splat gradient frame is what it was, through this hook too
    assert refusal_any(gsrt.MODE_COR | gsrt.FLAG_SPLAT_GRAD, 4) == (gsrt.OK, "")


def test_older_hooks_keep_their_callers_and_answers():
    """caller 5 stays GSRT_E_ARG through gsrt_debug_frame_refusal_kind and caller 4 through gsrt_debug_frame_refusal;
    the callers each of them has answer alike through all three hooks, the new bit included"""
    L = gsrt.lib
    assert L.gsrt_debug_frame_refusal_kind(gsrt.MODE_COR | gsrt.FLAG_SPLAT_DEPTH_GRAD, DEPTH, 1, 1, 0, 0, 0, None, 0) == gsrt.E_ARG
    assert L.gsrt_debug_frame_refusal(gsrt.MODE_COR, 4, 1, 1, 0, 0, 0, None, 0) == gsrt.E_ARG
    flags = (0, gsrt.FLAG_LUT, gsrt.FLAG_STATS, gsrt.FLAG_DEPTH, gsrt.FLAG_FEATURES, gsrt.FLAG_FEATURE_GRAD, gsrt.FLAG_SH_GRAD,
             gsrt.FLAG_OPACITY_GRAD, gsrt.FLAG_SPLAT_GRAD, gsrt.FLAG_SPLAT_DEPTH_GRAD, 0x10000, 0x40000,
             gsrt.FLAG_SPLAT_GRAD | gsrt.FLAG_LUT)
    for low in (gsrt.MODE_REF, gsrt.MODE_COR, 2):
        for f in flags:
            for caller in (0, 1, 2, 3, 4):
                for sh in (0, 1):
                    args = (low | f, caller, 1, 1, 0, 1, sh)
                    assert refusal_kind(*args) == refusal_any(*args), args
                    if caller < 4:
                        assert frame_refusal(*args) == refusal_any(*args), args


def test_cli_depth_grad_needs_the_splat_pair(tmp_path):
    """--depth-grad without --splat-grad: exit status 2 and the parser's message, before any device is opened"""
    import os
    import subprocess

    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(gsrt.__file__))), "bin", "gsrt_render")
    for argv in (["--scene", "100", "--depth-grad", "gd.bin"],
                 ["--scene", "100", "--depth-grad", "gd.bin", "--splat-grad-out", "o.bin"]):
        p = subprocess.run([cli] + argv, capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode == 2, (p.returncode, p.stderr)
        assert p.stderr.startswith("gsrt_render: --depth-grad goes with --splat-grad and --splat-grad-out"), p.stderr
        assert "[--depth-grad FILE]" in p.stderr and "gsrt_create" not in p.stderr
        assert not os.listdir(tmp_path)


@pytest.mark.gpu
def test_cli_depth_grad_writes_the_rows(tmp_path):
    """gsrt_render --splat-grad G --depth-grad GD --splat-grad-out FILE: n rows of 8 floats, slot 6 filled, slot 7 zero;
    without --depth-grad slot 6 stays zero"""
    import os
    import subprocess

    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(gsrt.__file__))), "bin", "gsrt_render")
    w, h, n = 32, 16, 500
    np.ones((h, w, 4), np.float32).tofile(tmp_path / "g.bin")
    np.ones((h, w), np.float32).tofile(tmp_path / "gd.bin")
    base = [cli, "--scene", "100", "--gaussians", str(n), "--width", str(w), "--height", str(h), "--samples", "1", "--no-dump",
            "--splat-grad", "g.bin"]
    for extra, out in ((["--depth-grad", "gd.bin"], "rows_d.bin"), ([], "rows.bin")):
        p = subprocess.run(base + extra + ["--splat-grad-out", out], capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode == 0, (p.stdout, p.stderr)
    rows_d = np.fromfile(tmp_path / "rows_d.bin", np.float32).reshape(-1, 8)
    rows = np.fromfile(tmp_path / "rows.bin", np.float32).reshape(-1, 8)
    assert rows_d.shape == rows.shape == (n, 8)
    assert (rows_d[:, 6] >= 0).all() and rows_d[:, 6].any() and not rows_d[:, 7].any() and not rows[:, 6:].any()


# ------------------------------------------------------------------------------------------------ gpu
W = H = 16
N = 100


def _scene(ctx, mesh=False):
    c, r, s, o, table = gsrt.synth_cloud(gsrt.SYNTH_COR, N, 9, True)
    sc = gsrt.Scene.from_model(ctx, c, r, s, np.minimum(o, np.float32(0.9)), table)
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
    G, Gd, rows = np.ones((H, W, 4), np.float32), np.ones((H, W), np.float32), np.zeros((N, 8), np.float32)
    gc, gv = np.zeros((N, 3), np.float32), np.zeros((N, 6), np.float32)
    d_G, d_Gd = torch.from_numpy(G).to("cuda:0"), torch.from_numpy(Gd).to("cuda:0")
    d_rows = torch.zeros((N, 8), dtype=torch.float32, device="cuda:0")
    d_c, d_v = torch.zeros((N, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((N, 6), dtype=torch.float32, device="cuda:0")
    p = gsrt._p
    F = gsrt.FLAG_SPLAT_DEPTH_GRAD
    sc = _scene(ctx)
    try:
        h = sc.handle
        # before the BVH is built
        assert L.gsrt_render_splat_depth_grad(h, u, gsrt.MODE_COR, 0, p(G), p(Gd), p(rows), 0) == gsrt.E_STATE
        assert L.gsrt_splat_depth_grad_to_model(h, u, p(rows), p(gc), p(gv), 0) == gsrt.E_STATE and "gsrt_build_bvh" in _last(ctx)
        sc.build_bvh()
        before = sc.render(ubo)[0].tobytes()

        def refused(status, want_status, *words):
            assert status == want_status, (status, _last(ctx))
            for w in words:
                assert w in _last(ctx), (w, _last(ctx))
            assert sc.render(ubo)[0].tobytes() == before

        # the flag through the other whole-frame entry points
        rgba, depth, t1 = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32), np.zeros(N, np.float32)
        refused(L.gsrt_render(h, u, gsrt.MODE_COR | F, 0, p(rgba), None), gsrt.E_ARG, FLAG, "only through " + ENTRY)
        refused(L.gsrt_render_async(h, u, gsrt.MODE_COR | F, 0, None, None), gsrt.E_ARG, FLAG)
        refused(L.gsrt_render_depth(h, u, gsrt.MODE_COR | F, 0, p(rgba), p(depth)), gsrt.E_ARG, FLAG)
        refused(L.gsrt_render_opacity_grad(h, u, gsrt.MODE_COR | F, 0, p(G), p(t1), 0), gsrt.E_ARG, FLAG)
        refused(L.gsrt_render_splat_grad(h, u, gsrt.MODE_COR | F, 0, p(G), p(rows), 0), gsrt.E_ARG, FLAG, "only through")
        # a sharded entry point
        refused(L.gsrt_render_sharded_emulated(h, u, gsrt.MODE_COR | F, 2, None, p(rgba)), gsrt.E_ARG, FLAG, "whole frames only")
        # LUT, REF, STATS and the other frame flags through the entry point itself, blocking and async
        for mode, word in ((gsrt.MODE_COR | gsrt.FLAG_LUT, "not with GSRT_FLAG_LUT"), (gsrt.MODE_REF, "COR frames only"),
                           (gsrt.MODE_COR | gsrt.FLAG_STATS, "not with GSRT_FLAG_STATS"),
                           (gsrt.MODE_COR | gsrt.FLAG_OUT_DUMP8, "not with GSRT_FLAG_OUT_DUMP8"),
                           (gsrt.MODE_COR | gsrt.FLAG_DEPTH, "not with GSRT_FLAG_DEPTH"),
                           (gsrt.MODE_COR | gsrt.FLAG_FEATURES, "not with GSRT_FLAG_FEATURES"),
                           (gsrt.MODE_COR | gsrt.FLAG_OPACITY_GRAD, "not with GSRT_FLAG_OPACITY_GRAD"),
                           (gsrt.MODE_COR | gsrt.FLAG_SH_GRAD, "not with GSRT_FLAG_SH_GRAD"),
                           (gsrt.MODE_COR | gsrt.FLAG_SPLAT_GRAD, "not with GSRT_FLAG_SPLAT_GRAD")):
            want = refusal_any(mode | F, DEPTH, sh=1)
            assert want == (gsrt.E_ARG, FLAG + ": " + word)
            refused(L.gsrt_render_splat_depth_grad(h, u, mode, 0, p(G), p(Gd), p(rows), 0), gsrt.E_ARG, want[1])
            refused(L.gsrt_render_splat_depth_grad_async(h, u, mode, 0, P(d_G.data_ptr()), P(d_Gd.data_ptr()),
                                                         P(d_rows.data_ptr()), 0), gsrt.E_ARG, want[1])
        # NULL images and tables
        refused(L.gsrt_render_splat_depth_grad(h, u, gsrt.MODE_COR, 0, None, p(Gd), p(rows), 0), gsrt.E_ARG, FLAG, "grad_image is NULL")
        refused(L.gsrt_render_splat_depth_grad(h, u, gsrt.MODE_COR, 0, p(G), None, p(rows), 0), gsrt.E_ARG, FLAG, "grad_depth is NULL")
        refused(L.gsrt_render_splat_depth_grad(h, u, gsrt.MODE_COR, 0, p(G), p(Gd), None, 0), gsrt.E_ARG, FLAG, "grad_table is NULL")
        refused(L.gsrt_render_splat_depth_grad_async(h, u, gsrt.MODE_COR, 0, P(d_G.data_ptr()), None, P(d_rows.data_ptr()), 0),
                gsrt.E_ARG, FLAG, "grad_depth is NULL")
        refused(L.gsrt_splat_depth_grad_to_model(h, u, None, p(gc), p(gv), 0), gsrt.E_ARG, "grad_splat is NULL")
        refused(L.gsrt_splat_depth_grad_to_model(h, u, p(rows), None, p(gv), 0), gsrt.E_ARG, "grad_center is NULL")
        refused(L.gsrt_splat_depth_grad_to_model(h, u, p(rows), p(gc), None, 0), gsrt.E_ARG, "grad_cov is NULL")
        refused(L.gsrt_splat_depth_grad_to_model_async(h, u, P(d_rows.data_ptr()), P(d_c.data_ptr()), None, 0), gsrt.E_ARG)
        assert L.gsrt_splat_depth_grad_to_model(None, u, p(rows), p(gc), p(gv), 0) == gsrt.E_ARG
        # a host table with accumulate
        refused(L.gsrt_render_splat_depth_grad(h, u, gsrt.MODE_COR, 0, p(G), p(Gd), p(rows), 1), gsrt.E_ARG, FLAG, "accumulate")
        refused(L.gsrt_splat_depth_grad_to_model(h, u, p(rows), p(gc), P(d_v.data_ptr()), 1), gsrt.E_ARG,
                "gsrt_splat_depth_grad_to_model", "accumulate")
        # and what is let through runs: host images, device images, a host image beside a device one
        assert L.gsrt_render_splat_depth_grad(h, u, gsrt.MODE_COR, 0, p(G), p(Gd), p(rows), 0) == gsrt.OK
        assert rows[:, :7].any(0).all() and not rows[:, 7].any()
        assert not ctx.slot_streams() and gsrt.lib.gsrt_depth_buffer(ctx.handle) is None
        assert gsrt.lib.gsrt_feature_buffer(ctx.handle) is None
        mixed = np.zeros((N, 8), np.float32)
        assert L.gsrt_render_splat_depth_grad(h, u, gsrt.MODE_COR, 0, P(d_G.data_ptr()), p(Gd), p(mixed), 0) == gsrt.OK
        assert np.allclose(mixed, rows, rtol=1e-4, atol=1e-6)
        assert L.gsrt_splat_depth_grad_to_model(h, u, p(rows), p(gc), p(gv), 0) == gsrt.OK and gc.any() and gv.any()
        assert L.gsrt_splat_depth_grad_to_model(h, u, P(d_rows.data_ptr()), P(d_c.data_ptr()), P(d_v.data_ptr()), 1) == gsrt.OK
        assert sc.render(ubo)[0].tobytes() == before
    finally:
        sc.close()


@pytest.mark.gpu
def test_a_scene_with_a_mesh_is_refused(ctx):
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 1, 16)
    u, p, L = gsrt._p(ubo), gsrt._p, gsrt.lib
    G, Gd, rows = np.ones((H, W, 4), np.float32), np.ones((H, W), np.float32), np.zeros((N, 8), np.float32)
    gc, gv = np.zeros((N, 3), np.float32), np.zeros((N, 6), np.float32)
    sc = _scene(ctx, mesh=True)
    try:
        sc.build_bvh()
        before = sc.render(ubo, gsrt.MODE_REF, raystate=True)[1].tobytes()
        assert L.gsrt_render_splat_depth_grad(sc.handle, u, gsrt.MODE_COR, 0, p(G), p(Gd), p(rows), 0) == gsrt.E_ARG
        assert _last(ctx) == FLAG + ": not for a scene with a triangle mesh"
        assert L.gsrt_splat_depth_grad_to_model(sc.handle, u, p(rows), p(gc), p(gv), 0) == gsrt.E_ARG
        assert "triangle mesh" in _last(ctx)
        assert sc.render(ubo, gsrt.MODE_REF, raystate=True)[1].tobytes() == before
    finally:
        sc.close()
