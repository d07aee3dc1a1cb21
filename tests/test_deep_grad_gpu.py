"""Every gradient kind, and the depth and feature frames, held to float64 where a tile's list continues: the scenes of
tests/deep_cases.py, whose tiles hold more candidates than their first list (kCap = 256 ids). The gradient tests beside
this one compare with a reference on scenes whose first list holds the whole tile; these run the rounds after it (the cut
list resumed in the group's list, the group list's second segment, the tile's own traversal past the list's end, with the
one-node restart under GSRT_DEBUG_STACK_LIMIT), the resweep kinds' second sweep over several rounds, and passes times rounds.

Every test first renders a plain frame with FLAG_STATS and asserts from the statistics how deep the device finds the
scene (`deep`): the fullest tile's candidate count, the candidates the rays went through, the rounds per tile, restarts
under the stack limit. A gradient test must not pass because the scene drifted shallow. That is a statement about the
scene, not an observation of the gradient frame's path: a counting frame keeps every AABB candidate and runs without
group lists (k_collect_cor, then the tile's own traversal), so it never runs round_from_group or k_group_more. A
gradient frame of the same scene resumes in its group's list, reads the second segment or traverses past the list's end
because of launch_render's conditions (group lists on every frame but a counting one; k_group_more where a tile holds 16
samples per pixel) together with the counts the device and tests/test_deep_grad_ref.py find; nothing in the library
reports which of them ran. The depth cull of an overflowed buffer is reached in `segment` alone (k_group_list and
k_group_more there); `traverse`, at 1 spp in 2x2 groups of 8x8-pixel tiles, runs without it. The scenes' conditions (the
float32-sensitive share, the candidate counts per tile and group, stops, clamps) and the comparison's power are asserted
on the CPU in tests/test_deep_grad_ref.py. References, upstream gradients (zero on the sensitive pixels) and bounds are the existing
ones: cor_f64.gradients, cor_f64_geom.splat_gradients and cor_f64_depth.depth_gradients through test_grad_f64_gpu's `hold`
(every entry within 1e-3 M, entries nothing reaches +0, the worst ratio printed and appended to COR_F64_REPORT) and
frame_checks; the forward frames as test_depth_gpu.py and test_features_gpu.py hold theirs. Measured ratios: DESIGN.md
section 5.
"""
import contextlib
import json
import os

import numpy as np
import pytest

import cor_f64 as F
import deep_cases as DC
import gsrt
import oracle as O
import test_depth_gpu as TD
import test_features_gpu as TF
import test_grad_f64_gpu as TG
from test_features_gpu import _d2h, u32

pytestmark = pytest.mark.gpu

TRAVERSE = ("traverse", 24, 16, 1)
# (case, GSRT_DEBUG_STACK_LIMIT): every case, and the one whose tiles traverse on their own again under the stack limit
RUNS = [(case, None) for case in DC.CASES] + [(TRAVERSE, "48")]
RUN = pytest.mark.parametrize("run", RUNS, ids=lambda r: DC.case_id(r[0]) + ("-stack48" if r[1] else ""))
# what the fullest tile's candidate count must exceed (`cut`: a second round as full as the first; `passes`: a full first
# list, the rounds per pass are counted), and how deep the median ray itself must go: past the first list; past the 896
# keys of a group list's first segment, where a gradient frame reads the second (segment) or the tile traverses on its own
# (traverse, 1 spp: no second segment). `traverse`'s rays stop in the opaque layer, near candidate 1700
TILE_BEYOND = {"cut": 2 * DC.K_CAP, "segment": DC.K_GCAP, "traverse": DC.K_GLIST, "passes": DC.K_CAP}
BEYOND = {"cut": DC.K_CAP, "segment": DC.K_GCAP, "traverse": DC.K_GCAP, "passes": DC.K_CAP}
MV = gsrt.lookat((0, 0, 0), (0, 0, -1))


def camera(case):
    _, w, h, spp = case
    ubo = gsrt.camera_from_modelview(MV, DC.FOVY, w, h, 1.0, spp, 16)
    want = DC.camera(case)  # what the CPU scene conditions were asserted under
    assert all(np.array_equal(ubo[k], want[k]) for k in ("model_view", "projection", "width", "height", "samples",
                                                          "random_seed"))
    plan = gsrt.tile_plan(ubo)
    assert (plan["tile_w"], plan["tile_h"], plan["spp_lanes"]) == DC.kernel_tile(spp)
    return ubo


@contextlib.contextmanager
def deep(ctx, monkeypatch, run, rows="own"):
    """The case's scene (with its SH rows, without any, or with the rows given) and camera, after the proof from a plain
    FLAG_STATS frame that the case's path ran; under the stack limit also that tiles restarted and that the plain frame's
    bytes are those without it."""
    case, limit = run
    c, r, s, o, sh = DC.model(case)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh if isinstance(rows, str) and rows == "own" else rows)
    try:
        sc.build_bvh()
        ubo = camera(case)
        if limit:
            before = sc.render(ubo, gsrt.MODE_COR)[0]
            monkeypatch.setenv("GSRT_DEBUG_STACK_LIMIT", limit)
            assert sc.render(ubo, gsrt.MODE_COR)[0].tobytes() == before.tobytes()
        sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_STATS)
        st = ctx.last_stats((case[2], case[1]))
        # A counting frame keeps every AABB candidate (no footprint cull, no depth cull) and runs without group lists:
        # k_collect_cor writes the tile's first list, every later round is the tile's own traversal. max_tile_candidates
        # is the largest `total` of a round: round_from_list reports its count (256 at most), a traversal round the keys
        # left beyond the previous round's last. So it is max(256, the fullest tile's candidates - 256): 881 for the 1137
        # of `segment`, 256 for `passes` (fewer than 256 are left for the second round). Plus 256 it is that tile's count
        shown = st["max_tile_candidates"] + DC.K_CAP
        assert st["max_tile_candidates"] >= DC.K_CAP and shown > TILE_BEYOND[case[0]], st
        # and the rays themselves: the candidates a ray's slab test passed before the ray stopped, summed over the pixel's
        # samples. The median pixel's mean over its samples (a ray through a clamped Gaussian stops early) lies beyond the
        # first list, or beyond 896, where a gradient frame's group list ends its first segment
        per_sample = st.pop("per_ray")[..., 0].astype(np.int64) // case[3]
        assert np.median(per_sample) > BEYOND[case[0]], (np.median(per_sample), st)
        assert st["tile_rounds"] > st["tiles"], st
        if case[3] > 64:
            assert st["tile_rounds"] >= 2 * case[3] * st["tiles"], st  # more than one round in every pass
        if limit:
            assert st["restarts"] > 0, st
        yield sc, ubo
    finally:
        sc.close()


def label_of(label, run):
    return label + (" stack 48" if run[1] else "")


def report(label, case, entries, near, worst):
    rep = os.environ.get("COR_F64_REPORT")
    if rep:
        with open(rep, "a") as fh:
            fh.write(json.dumps({"case": "%s %s %dx%d spp %d" % ((label,) + case), "entries": int(entries),
                                 "sensitive_frac": round(float(near.mean()), 5), "worst_ratio": float(worst)}) + "\n")


# ------------------------------------------------------------------------------------------------ gradient kinds
@RUN
def test_opacity_grad_with_sh_matches_f64(ctx, monkeypatch, run):
    case = run[0]
    G, ref, want = DC.reference(case, True)
    with deep(ctx, monkeypatch, run) as (sc, ubo):
        got = sc.opacity_grad(ubo, G)
        TG.frame_checks(ctx, sc, ubo, case, want)
    TG.hold(label_of("deep opacity-grad SH", run), case, ref.near, got, ref.opacity, ref.M_opacity)


@RUN
def test_opacity_grad_without_sh_matches_f64(ctx, monkeypatch, run):
    case = run[0]
    G, ref, want = DC.reference(case, False)
    with deep(ctx, monkeypatch, run, rows=None) as (sc, ubo):
        got = sc.opacity_grad(ubo, G)
        TG.frame_checks(ctx, sc, ubo, case, want)
    TG.hold(label_of("deep opacity-grad colour 1", run), case, ref.near, got, ref.opacity, ref.M_opacity)


@RUN
def test_sh_grad_matches_f64(ctx, monkeypatch, run):
    case = run[0]
    G, ref, want = DC.reference(case, True)
    with deep(ctx, monkeypatch, run) as (sc, ubo):
        got = sc.sh_grad(ubo, G)
        TG.frame_checks(ctx, sc, ubo, case, want)
    assert 0 < ref.counts["channels_clamped"] < ref.counts["channels"]
    TG.hold(label_of("deep sh-grad", run), case, ref.near, got, ref.sh, ref.M_sh)


def feature_check(ctx, monkeypatch, run, channels):
    """The frame's RGBA is the feature frame's: the scene's frame without SH rows."""
    case = run[0]
    G, ref = DC.feature_reference(case, channels)
    want = DC.reference(case, False)[2]
    c, r, s, o, _ = DC.model(case)
    bare = gsrt.Scene.from_model(ctx, c, r, s, o)
    try:
        bare.build_bvh()
        with deep(ctx, monkeypatch, run) as (sc, ubo):  # SH rows in the scene: a feature gradient frame ignores them
            got = sc.feature_grad(ubo, G)
            fb = _d2h(ctx.framebuffer_ptr, (case[2], case[1], 4))
            assert fb.tobytes() == bare.render(ubo, gsrt.MODE_COR)[0].tobytes()
            assert np.abs(fb.astype(np.float64) - want).max() <= 1e-3
    finally:
        bare.close()
    TG.hold(label_of("deep feature-grad C=%d" % channels, run), case, ref.near, got, ref.feat, ref.M_feat)


@RUN
def test_feature_grad_matches_f64(ctx, monkeypatch, run):
    feature_check(ctx, monkeypatch, run, 5)


def test_feature_grad_16_channels_matches_f64(ctx, monkeypatch):
    feature_check(ctx, monkeypatch, (DC.CASES[0], None), gsrt.MAX_FEATURES)


@RUN
def test_splat_rows_match_f64(ctx, monkeypatch, run):
    case = run[0]
    n = len(DC.model(case)[3])
    G, sg = DC.splat_reference(case, True)
    with deep(ctx, monkeypatch, run) as (sc, ubo):
        got = sc.splat_grad(ubo, G)
        TG.frame_checks(ctx, sc, ubo, case, DC.reference(case, True)[2])
    assert got.shape == (n, 8) and got.dtype == np.float32
    assert not u32(got[:, 6:]).any()  # slots 6 and 7: all bits zero
    TG.hold(label_of("deep splat-grad SH", run), case, sg.near, got[:, :6], sg.rows[:, :6], sg.M[:, :6])


@RUN
def test_splat_depth_rows_match_f64(ctx, monkeypatch, run):
    case = run[0]
    n = len(DC.model(case)[3])
    G, Gd, dg = DC.depth_reference(case, True)
    with deep(ctx, monkeypatch, run) as (sc, ubo):
        got = sc.splat_depth_grad(ubo, G, Gd)
        TG.frame_checks(ctx, sc, ubo, case, DC.reference(case, True)[2])
    assert got.shape == (n, 8) and got.dtype == np.float32
    assert not u32(got[:, 7]).any()  # slot 7: all bits zero
    assert np.abs(dg.rows[:, 6]).max() > 0
    TG.hold(label_of("deep splat-depth-grad SH", run), case, dg.near, got[:, :7], dg.rows[:, :7], dg.M[:, :7])


# ------------------------------------------------------------------------------------------------ forward kinds
def oracle_frame(case, rows):
    c, r, s, o, _ = DC.model(case)
    p, a = O.gauss_from_model(c, r, s, o)
    ref = O.render(p, a, DC.camera(case), O.MODE_COR, sh=rows, bvh=O.Bvh(a), want_stats=True, threads=4)
    return ref["rgba"], ref["stats"].astype(np.int64)


@RUN
def test_depth_frame_matches_the_oracle_and_f64(ctx, monkeypatch, run):
    """As test_depth_of_clouds_matches_the_oracle (the frame's bytes are the oracle's, the depth within delta + 2 n_max
    2^-24 z_max of the oracle's depth-coloured frame) and test_depth_matches_f64 (L-inf <= 1e-3 z_max on every pixel)."""
    case = run[0]
    c, r, s, o, _ = DC.model(case)
    z = -c[:, 2]
    rows = TD.depth_rows(z)
    want, st = oracle_frame(case, rows)
    z_max = float(z.max())
    tol = TD.encoding_cost(z) + 2.0 * float(st[..., 1].max()) * 2.0 ** -24 * z_max
    with deep(ctx, monkeypatch, run, rows=rows) as (sc, ubo):
        plain, _ = sc.render(ubo, gsrt.MODE_COR)
        rgba, depth = sc.render_depth(ubo, gsrt.MODE_COR)
    assert rgba.tobytes() == plain.tobytes() and rgba.tobytes() == want.tobytes()
    linf = float(np.abs(depth.astype(np.float64) - want[..., 0].astype(np.float64)).max())
    want64, near = F.render(DC.camera(case), c, r, s, o, TD.depth_rows(z.astype(np.float64), np.float64))
    diff = np.abs(depth.astype(np.float64) - want64[..., 0])
    print(f"deep depth {run}: vs oracle L-inf {linf:.3g}, tol {tol:.3g} (n_max {st[..., 1].max()}); vs f64 L-inf "
          f"{diff.max():.3g}, bound {1e-3 * z_max:.3g}, {near.mean():.2%} of the pixels float32-sensitive")
    report(label_of("deep depth frame", run), case, diff.size, near, diff.max() / (1e-3 * z_max))
    assert linf <= tol
    assert np.abs(rgba[..., 3].astype(np.float64) - want64[..., 3]).max() <= 1e-3
    assert diff.max() <= 1e-3 * z_max


@RUN
def test_feature_frame_matches_the_oracle_and_f64(ctx, monkeypatch, run):
    """As test_features_of_clouds_match_the_oracle (six channels against the oracle's frames coloured by three of them at
    a time) and test_features_match_f64 (L-inf <= 1e-3 f_max on every pixel and channel, here on the first three)."""
    case = run[0]
    c, r, s, o, _ = DC.model(case)
    table = TF.noise(len(o), 6, 31, 0.0, 8.0)
    f_max = float(table.max())
    with deep(ctx, monkeypatch, run, rows=None) as (sc, ubo):
        sc.set_features(table)
        plain, _ = sc.render(ubo, gsrt.MODE_COR)
        rgba, feat = sc.render_features(ubo)
    assert rgba.tobytes() == plain.tobytes()
    for g in range(2):
        cols = table[:, 3 * g:3 * g + 3]
        want, st = oracle_frame(case, TF.feature_rows(cols))
        assert np.array_equal(u32(want[..., 3]), u32(rgba[..., 3]))  # the same hits
        tol = TF.encoding_cost(cols) + 2.0 * float(st[..., 1].max()) * 2.0 ** -24 * f_max
        linf = float(np.abs(feat[..., 3 * g:3 * g + 3].astype(np.float64) - want[..., :3].astype(np.float64)).max())
        print(f"deep features {run} channels {3 * g}..{3 * g + 2}: vs oracle L-inf {linf:.3g}, tol {tol:.3g}")
        assert linf <= tol
    want64, near = F.render(DC.camera(case), c, r, s, o, TF.feature_rows(table[:, :3].astype(np.float64), np.float64))
    diff = np.abs(feat[..., :3].astype(np.float64) - want64[..., :3])
    print(f"deep features {run}: vs f64 L-inf {diff.max():.3g}, bound {1e-3 * f_max:.3g}, {near.mean():.2%} sensitive")
    report(label_of("deep feature frame", run), case, diff.size, near, diff.max() / (1e-3 * f_max))
    assert np.abs(rgba[..., 3].astype(np.float64) - want64[..., 3]).max() <= 1e-3
    assert diff.max() <= 1e-3 * f_max
