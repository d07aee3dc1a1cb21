"""Stage boundaries of the COR shading loop (shade_sorted / shade_stage): bit-exact against the CPU oracle.

The loop shades a tile's sorted list in stages of kGroup = 4 candidates: a steady-state loop over whole stage triples
while 4 more stages' worth of list lies ahead, and the general code for the rest. The scenes here control the list
length of every tile and where rays stop, and each asserts from the oracle's per-ray counts (candidates, blends,
stops) that it still exercises the boundary it is meant for.

Scenes are small stacks of Gaussians in front of a camera at the origin looking down -z, every AABB covering the whole
frame unless said otherwise: then every ray's candidate list is the tile's list, and a ray that stops at its j-th
candidate stops at list position j - 1.
"""
import numpy as np
import pytest

import gsrt
import oracle as O

pytestmark = pytest.mark.gpu

K_GROUP = 4   # candidates per LDS stage (kGroup)
K_CAP = 256   # list entries per round (kCap)
FOV = 60.0
IDENT = (1.0, 0.0, 0.0, 0.0)


def stack(k, opacity, scale=3.0, spread=0.0, seed=1):
    """k Gaussians on the view axis at depths 5, 5.01, ... (sorted order = index order), isotropic `scale`, centres
    moved sideways by up to `spread` (uniform, seeded)."""
    rng = np.random.default_rng(seed)
    c = np.zeros((k, 3), np.float32)
    c[:, 2] = -5.0 - 0.01 * np.arange(k, dtype=np.float32)
    c[:, :2] = rng.uniform(-spread, spread, (k, 2)).astype(np.float32) if spread else 0.0
    r = np.tile(np.asarray(IDENT, np.float32), (k, 1))
    s = np.full((k, 3), scale, np.float32)
    o = np.full(k, opacity, np.float32)
    return c, r, s, o


def sh_rows(k, seed=3):
    """SH-3 coefficients of the synthetic cloud (signed, so the clamp at 0 is met) for k Gaussians"""
    return gsrt.synth_cloud(gsrt.SYNTH_COR, max(k, 1), seed, True)[4][:k]


def mixed_layouts(k):
    """Alternating in depth order: a box in the octant x > 0, y > 0, z < 0 of the camera origin (the ordered record
    layout) and a box that straddles the origin's x and y planes (the general layout)."""
    c = np.zeros((k, 3), np.float32)
    c[:, 2] = -5.0 - 0.01 * np.arange(k, dtype=np.float32)
    s = np.full((k, 3), 3.0, np.float32)
    c[0::2, :2] = 1.2
    s[0::2] = 0.3
    r = np.tile(np.asarray(IDENT, np.float32), (k, 1))
    o = np.full(k, 0.3, np.float32)
    return c, r, s, o


def one_sided(aabbs):
    """per box: on one side of the camera origin (0, 0, 0) on every axis"""
    return np.all((aabbs[:, :3] > 0) | (aabbs[:, 3:] < 0), axis=1)


def render_both(ctx, model, sh, w, h, spp):
    """(GPU frame, oracle frame, oracle per-pixel counts [candidates, blends, -, stops], aabbs)"""
    c, r, s, o = model
    mv = gsrt.lookat((0, 0, 0), (0, 0, -1))
    if len(o):
        sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    else:
        sc = gsrt.Scene.from_params(ctx, np.zeros((0, 12), np.float32), np.zeros((0, 6), np.float32))
        sh = None
    try:
        sc.build_bvh()
        p, a = sc.download()
        rgba, _ = sc.render(gsrt.camera_from_modelview(mv, FOV, w, h, 1.0, spp, 16), gsrt.MODE_COR)
    finally:
        sc.close()
    ref = O.render(p, a, O.make_ubo(mv, FOV, w, h, 1.0, spp, 16), O.MODE_COR, sh=sh, bvh=O.Bvh(a) if len(o) else None,
                   want_stats=True, threads=4)
    return rgba, ref["rgba"], ref["stats"].astype(np.int64), a


@pytest.mark.parametrize("spp", [4, 1])
@pytest.mark.parametrize("with_sh", [False, True])
def test_every_list_length(ctx, with_sh, spp):
    """Lists of 0..25 entries in every tile: empty, shorter than three stages (the steady-state loop is not entered),
    one steady-state trip (17 or more entries) with a remainder of one to three stages, a last stage of 1..4."""
    assert 3 * K_GROUP * 2 + 1 == 25
    for k in range(0, 26):
        rgba, want, st, _ = render_both(ctx, stack(k, 0.05), sh_rows(k) if with_sh else None, 16, 16, spp)
        # every ray meets all k boxes (so every tile's list has k entries), blends some and never stops
        assert (st[..., 0] == k * spp).all(), k
        assert (st[..., 3] == 0).all(), k
        assert k == 0 or st[..., 1].min() > 0, k
        assert rgba.tobytes() == want.tobytes(), f"list length {k}"


@pytest.mark.parametrize("with_sh", [False, True])
def test_stop_inside_a_stage(ctx, with_sh):
    """Opaque Gaussians (0.99) moved sideways: the rays of one wave stop at different candidates, at every position
    of a stage, while other lanes of the wave go on blending the same stage's later candidates."""
    k = 22
    rgba, want, st, _ = render_both(ctx, stack(k, 0.99, scale=1.6, spread=1.3, seed=7),
                                    sh_rows(k) if with_sh else None, 16, 16, 1)
    ncand, nblend, nstop = st[..., 0], st[..., 1], st[..., 3]
    stopped = nstop == 1
    assert (ncand[~stopped] == k).all()  # a ray that never stops walks the whole list: its boxes are the tile's list
    assert stopped.sum() > 64
    pos = ncand - 1  # list position of the stop (1 spp: one ray per pixel)
    assert set((pos[stopped] % K_GROUP).tolist()) == {0, 1, 2, 3}
    # in one 8x8 tile (one wave at 1 spp): two rays stop in the same stage at different positions, and the later
    # one has blended since the earlier one stopped
    found = False
    for ty in range(0, 16, 8):
        for tx in range(0, 16, 8):
            m = stopped[ty:ty + 8, tx:tx + 8]
            pp, nb = pos[ty:ty + 8, tx:tx + 8][m], nblend[ty:ty + 8, tx:tx + 8][m]
            for stage in np.unique(pp // K_GROUP):
                sel = pp // K_GROUP == stage
                if np.unique(pp[sel]).size >= 2 and nb[sel].max() > nb[sel].min():
                    found = True
    assert found
    assert rgba.tobytes() == want.tobytes()


@pytest.mark.parametrize("spp", [4, 1])
def test_both_record_layouts_in_one_stage(ctx, spp):
    k = 14
    model = mixed_layouts(k)
    rgba, want, st, a = render_both(ctx, model, sh_rows(k), 16, 16, spp)
    side = one_sided(a)
    assert side[0::2].all() and not side[1::2].any()  # adjacent list positions alternate between the layouts
    # rays through the small boxes meet both kinds (more candidates than the k / 2 straddling boxes) and blend both
    assert st[..., 0].max() == k * spp and st[..., 0].min() == (k // 2) * spp
    assert st[..., 1].max() > (k // 2) * spp
    assert rgba.tobytes() == want.tobytes()


@pytest.mark.parametrize("spp", [4, 1])
def test_ragged_frame(ctx, spp):
    """18x18: the tiles of the last column and row hold lanes without a pixel (inactive from the start)."""
    pl = gsrt.tile_plan(gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), FOV, 18, 18, 1.0, spp, 16))
    assert 18 % pl["tile_w"] and 18 % pl["tile_h"]
    for k, op, spread in [(19, 0.05, 0.0), (22, 0.99, 1.3)]:
        rgba, want, st, _ = render_both(ctx, stack(k, op, scale=3.0 if op < 0.5 else 1.6, spread=spread, seed=7),
                                        sh_rows(k), 18, 18, spp)
        assert st[..., 0].max() == k * spp
        assert (st[..., 3].max() > 0) == (op > 0.5)
        assert rgba.tobytes() == want.tobytes()


def test_continuation_round(ctx):
    """More than kCap contributing candidates in every tile: a second round runs through the same loops."""
    k = 300
    rgba, want, st, _ = render_both(ctx, stack(k, 0.02, scale=6.0), sh_rows(k), 16, 16, 4)
    assert (st[..., 0] == k * 4).all() and (st[..., 3] == 0).all()
    assert st[..., 1].min() > K_CAP * 4  # every pixel's rays blend past the first round's kCap entries
    assert rgba.tobytes() == want.tobytes()
