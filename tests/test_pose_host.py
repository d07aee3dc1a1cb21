"""Host side of the pose gradient (no device): gsrt_pose_twist and gsrt_ubo_apply_twist against the float64 reference of
tests/cor_f64_pose.py, the exports, NULL refusals, and the shape errors of the Python wrappers.

"To one float32 rounding": the library computes in double and rounds once, so a result is within half a float32 ulp of the
exact value, |got - ref| <= 2^-24 |ref|, plus the two double computations' own difference, bounded here by 1e-13 of the
largest magnitude that enters the entry's sum.
"""
import ctypes

import numpy as np
import pytest

import cor_f64_pose as PQ
import gsrt
import pose_cases as PC

EPS = 2.0 ** -24
PI = float(np.pi)
TWISTS = [(0.0, 0.0, 0.0, 0.0, 0.0, 1e-8), (0.3, -0.2, 0.1, 1e-8, 0.0, 0.0), (0.1, 0.2, -0.3, 0.6, 0.0, 0.8),
          (0.05, 0.0, 0.2, 0.0, PI, 0.0), (0.0, 0.0, 0.0, 0.02, -0.03, 0.05), (0.5, 0.5, 0.5, 0.0, 0.0, 0.0),
          (0.2, -0.1, 0.4, PI * 0.6, 0.0, PI * 0.8)]  # |w| = 0, 1e-8, 1, pi, inside the series' range, and pi again


def test_exports_and_layout():
    assert {"gsrt_pose_grad", "gsrt_pose_grad_async", "gsrt_pose_twist", "gsrt_ubo_apply_twist",
            "gsrt_debug_pose_grad_layout"} <= set(gsrt.EXPORTS)
    assert gsrt.pose_grad_layout() == (PC.CHUNK, PC.LANES)
    assert gsrt.lib.gsrt_abi_version() == 2


def test_pose_twist_matches_f64():
    rng = np.random.default_rng(11)
    for ubo in (PC.camera(), PC.nonaffine_camera()):
        mv = ubo["model_view"][0]
        g = rng.normal(0.0, 3.0, 16).astype(np.float32)
        got = gsrt.pose_twist(mv, g)
        assert got.shape == (6,) and got.dtype == np.float32
        MV, G = PQ.mat(mv), PQ.mat(g)
        ref = PQ.twist(MV, G)
        mag = np.abs(G) @ np.abs(MV).T
        slack = 1e-13 * np.array([mag[0, 3], mag[1, 3], mag[2, 3], mag[2, 1] + mag[1, 2], mag[0, 2] + mag[2, 0], mag[1, 0] + mag[0, 1]])
        assert (np.abs(got.astype(np.float64) - ref) <= EPS * np.abs(ref) + slack).all()
        assert np.array_equal(gsrt.pose_twist(mv.reshape(4, 4), g.reshape(4, 4)), got)


@pytest.mark.parametrize("xi", TWISTS, ids=lambda t: "w%.3g" % np.linalg.norm(t[3:]))
def test_apply_twist_matches_f64(xi):
    for ubo in (PC.camera(), PC.nonaffine_camera()):
        got = gsrt.ubo_apply_twist(ubo, xi)
        xi64 = np.asarray(np.asarray(xi, np.float32), np.float64)  # the library is handed float32
        MV, MVi = PQ.mat(ubo["model_view"][0]), PQ.mat(ubo["model_view_inverse"][0])
        A, Ai = PQ.apply_twist(MV, MVi, xi64)
        E, Ei = np.abs(PQ.expm(PQ.hat(xi64))), np.abs(PQ.expm(-PQ.hat(xi64)))
        for name, want, mag in (("model_view", A, E @ np.abs(MV)), ("model_view_inverse", Ai, np.abs(MVi) @ Ei)):
            g = PQ.mat(got[name][0])
            assert (np.abs(g - want) <= EPS * np.abs(want) + 1e-13 * mag).all(), name
        # MV' MVinv' = exp(xi^) (MV MVinv) exp(-xi^) as far as the two float32 roundings allow, and that is I as far as
        # the ubo's own float32 inverse was one
        prod = PQ.mat(got["model_view"][0]) @ PQ.mat(got["model_view_inverse"][0])
        assert (np.abs(prod - A @ Ai) <= 2.01 * EPS * (np.abs(A) @ np.abs(Ai)) + 1e-12).all()
        assert (np.abs(A @ Ai - np.eye(4)) <= E @ np.abs(MV @ MVi - np.eye(4)) @ Ei + 1e-12).all()
        assert np.abs(prod - np.eye(4)).max() <= 1e-5
        for k in got.dtype.names:  # nothing else of the ubo moves
            if k not in ("model_view", "model_view_inverse"):
                assert got[k].tobytes() == ubo[k].tobytes()
        assert ubo["model_view"].tobytes() != got["model_view"].tobytes()


def test_zero_twist_keeps_every_bit():
    ubo = PC.nonaffine_camera()
    ubo["model_view"][0][5] = np.float32(-0.0)
    ubo["model_view_inverse"][0][2] = np.float32(np.nan)
    for xi in (np.zeros(6, np.float32), np.array([0.0, -0.0, 0.0, -0.0, 0.0, 0.0], np.float32)):
        assert gsrt.ubo_apply_twist(ubo, xi).tobytes() == ubo.tobytes()


def test_null_refusals():
    L, p = gsrt.lib, gsrt._p
    a, b, t = np.zeros(16, np.float32), np.zeros(16, np.float32), np.full(6, 7.0, np.float32)
    ubo = PC.camera()
    before = ubo.tobytes()
    assert L.gsrt_pose_twist(None, p(b), p(t)) == gsrt.E_ARG and L.gsrt_pose_twist(p(a), None, p(t)) == gsrt.E_ARG
    assert L.gsrt_pose_twist(p(a), p(b), None) == gsrt.E_ARG and (t == 7.0).all()
    assert L.gsrt_ubo_apply_twist(None, p(t)) == gsrt.E_ARG and L.gsrt_ubo_apply_twist(p(ubo), None) == gsrt.E_ARG
    assert ubo.tobytes() == before
    assert L.gsrt_debug_pose_grad_layout(None) == gsrt.E_ARG
    out = np.full(16, 3.0, np.float32)
    assert L.gsrt_pose_grad(None, p(ubo), p(a), 0, p(out)) == gsrt.E_ARG
    assert L.gsrt_pose_grad_async(None, p(ubo), ctypes.c_void_p(16), 0, ctypes.c_void_p(16)) == gsrt.E_ARG
    assert (out == 3.0).all()


def test_wrapper_shape_errors():
    ubo = PC.camera()
    for bad in (np.zeros(15), np.zeros((3, 4)), np.zeros(17)):
        with pytest.raises(gsrt.GsrtError):
            gsrt.pose_twist(bad, np.zeros(16))
        with pytest.raises(gsrt.GsrtError):
            gsrt.pose_twist(np.zeros(16), bad)
    for bad in (np.zeros(5), np.zeros(7), np.zeros((2, 4))):
        with pytest.raises(gsrt.GsrtError):
            gsrt.ubo_apply_twist(ubo, bad)
    with pytest.raises(gsrt.GsrtError):
        gsrt.ubo_apply_twist(np.zeros(16, np.float32), np.zeros(6))
    with pytest.raises(gsrt.GsrtError):
        gsrt.ubo_apply_twist(np.zeros(2, gsrt.UBO_DTYPE), np.zeros(6))
