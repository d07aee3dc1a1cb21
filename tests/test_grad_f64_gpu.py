"""The three gradient kernels (opacity, SH and feature gradient frames) against the independent float64 backward,
tests/cor_f64.py's gradients(): derived from the blend's definition, sharing no value with the forward kernel.

The gradient tests beside this one (test_feature_grad_gpu.py, test_sh_grad_gpu.py, test_opacity_grad_gpu.py) build their
references from the forward kernel's own weights, basis and depth order: tight float32 rounding bounds, but blind to
whatever forward and backward share, and limited to inputs whose clamps are decidable from the tables. The scene here
(test_grad_f64.scene; its conditions are asserted on the CPU in test_grad_f64.py) has alpha clamped at 0.99 behind other
hits, colour channels clamped at 0 on some of a Gaussian's rays and open on others, and rays that stop.

G is noise, set to zero on the pixels where float32 may take a decision the other way (F's `near`) before the kernel
runs; nothing is left out of the assertion, every table entry is held to
    |got - ref| <= 1e-3 M,   M the sum of the absolute values of the terms the entry sums (F.gradients),
the project's 1e-3 criterion (BASELINE.json; LINF in test_cor_independent.py) applied to an entry's magnitude. Entries
with M == 0 must be +0. Each test prints its worst error / (1e-3 M); with COR_F64_REPORT=<path> it appends a line to that
JSON-lines file, as test_cor_independent._check does. Measured ratios: DESIGN.md section 5.

Every frame is at most 48x32 pixels over 300 Gaussians.
"""
import json
import os

import numpy as np
import pytest

import cor_f64 as F
import gsrt
import test_grad_f64 as S
import test_sh_grad_gpu as TS
from test_features_gpu import MV, _d2h, u32, ubo_of

pytestmark = pytest.mark.gpu

TOL = S.TOL
CASES = pytest.mark.parametrize("case", S.CASES, ids=lambda c: "%s-%dx%d-spp%d" % c)
_REF = {}


def camera(case):
    cam, w, h, spp = case
    ubo = ubo_of(w, h, spp, MV if cam == "origin" else TS.MOVED)
    want = S.camera(*case)  # what the CPU scene conditions were asserted under
    assert all(np.array_equal(ubo[k], want[k]) for k in ("model_view", "projection", "width", "height", "samples",
                                                          "random_seed"))
    assert (gsrt.tile_plan(ubo)["spp_lanes"] != spp) == (spp == 3)  # 3 spp run as passes
    return ubo


def reference(case, with_sh):
    """G (zero on the sensitive pixels), F.gradients of it, and F.render's frame; computed once per case"""
    key = (case, with_sh)
    if key not in _REF:
        c, r, s, o, sh = S.scene()
        G = S.upstream(case, 4, 201 + case[3], with_sh)
        rows = sh if with_sh else None
        _REF[key] = (G, F.gradients(camera(case), c, r, s, o, rows, G_rgba=G), F.render(camera(case), c, r, s, o, rows)[0])
    return _REF[key]


def hold(label, case, near, got, ref, M):
    """every entry within TOL M of the reference; entries nothing reaches are +0"""
    got64 = np.asarray(got, np.float64)
    assert got64.shape == ref.shape and np.isfinite(got64).all()
    err = np.abs(got64 - ref)
    reached = M > 0
    worst = float((err[reached] / (TOL * M[reached])).max())
    print(f"{label} {case}: {reached.sum()} of {M.size} entries reached, {near.mean():.2%} of the pixels float32-sensitive; "
          f"worst error / (1e-3 M) = {worst:.3g}")
    rep = os.environ.get("COR_F64_REPORT")
    if rep:
        with open(rep, "a") as fh:
            fh.write(json.dumps({"case": "%s %s %dx%d spp %d" % ((label,) + case), "entries": int(M.size),
                                 "sensitive_frac": round(float(near.mean()), 5), "worst_ratio": worst}) + "\n")
    assert not u32(got)[~reached].any(), label
    assert (err <= TOL * M).all(), f"{label}: worst error / (1e-3 M) = {worst:.3g}"
    assert reached.sum() > M.size // 4


def frame_checks(ctx, sc, ubo, case, want64):
    """the gradient frame left the plain frame's bytes in the framebuffer, and they are within 1e-3 of F.render"""
    _, w, h, _ = case
    fb = _d2h(ctx.framebuffer_ptr, (h, w, 4))
    assert fb.tobytes() == sc.render(ubo, gsrt.MODE_COR)[0].tobytes()
    assert np.abs(fb.astype(np.float64) - want64).max() <= 1e-3


@CASES
def test_opacity_grad_with_sh_matches_f64(ctx, case):
    c, r, s, o, sh = S.scene()
    G, ref, want = reference(case, True)
    ubo = camera(case)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        got = sc.opacity_grad(ubo, G)
        frame_checks(ctx, sc, ubo, case, want)
    finally:
        sc.close()
    hold("opacity-grad SH", case, ref.near, got, ref.opacity, ref.M_opacity)


@CASES
def test_opacity_grad_without_sh_matches_f64(ctx, case):
    c, r, s, o, _ = S.scene()
    G, ref, want = reference(case, False)
    ubo = camera(case)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o)
    try:
        sc.build_bvh()
        got = sc.opacity_grad(ubo, G)
        frame_checks(ctx, sc, ubo, case, want)
    finally:
        sc.close()
    hold("opacity-grad colour 1", case, ref.near, got, ref.opacity, ref.M_opacity)


@CASES
def test_sh_grad_matches_f64(ctx, case):
    c, r, s, o, sh = S.scene()
    G, ref, want = reference(case, True)
    ubo = camera(case)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        got = sc.sh_grad(ubo, G)
        frame_checks(ctx, sc, ubo, case, want)
    finally:
        sc.close()
    assert ref.counts["mixed_pairs"] >= 100
    hold("sh-grad", case, ref.near, got, ref.sh, ref.M_sh)


@CASES
def test_feature_grad_matches_f64(ctx, case):
    """C = 5. The frame's RGBA is the feature frame's: the scene's frame without SH rows."""
    c, r, s, o, sh = S.scene()
    G = S.upstream(case, 5, 301 + case[3], with_sh=False)
    ubo = camera(case)
    ref = F.gradients(ubo, c, r, s, o, G_feat=G)
    want = reference(case, False)[2]
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)  # SH rows in the scene: a feature gradient frame ignores them
    bare = gsrt.Scene.from_model(ctx, c, r, s, o)
    try:
        sc.build_bvh()
        bare.build_bvh()
        got = sc.feature_grad(ubo, G)
        fb = _d2h(ctx.framebuffer_ptr, (case[2], case[1], 4))
        assert fb.tobytes() == bare.render(ubo, gsrt.MODE_COR)[0].tobytes()
        assert np.abs(fb.astype(np.float64) - want).max() <= 1e-3
    finally:
        sc.close()
        bare.close()
    hold("feature-grad", case, ref.near, got, ref.feat, ref.M_feat)
