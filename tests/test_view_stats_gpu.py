"""gsrt_view_stats_add on the GPU: the densification statistic and the largest screen radius from synthetic splat rows over
a synthetic model (tests/view_stats_ref.py; the rows are an input, so no frame is rendered).

n in {1, 257, 1000}: one lane, the 256-lane workgroup edge, and a tail. About a third of the rows are all +0, some hold
only a -0 (not seen), some a NaN (seen); two Gaussians lie behind the camera and one has a NaN covariance (singular), all
three with non-zero rows; radii starts as a mix of +0, 1e4 and a NaN pattern.

stats must be gsrt.density_stats_add's bits; untouched words keep theirs. The radius must be the ceil of the float64
reference's x = 3 sqrt(lam), except where x lies within the band of an integer: there a difference of 1 passes. The band is
8 x the largest relative difference between the float32 restatement and the float64 reference over these cases, measured on
the CPU (tests/test_view_stats_ref.py): 8 x 5e-7 (measured 4.95e-7) = 4e-6 relative to x. At most 2 % of the seen valid
Gaussians may lie in it; with this seed none of the 764 does."""
import ctypes

import numpy as np
import pytest

import gsrt
import view_stats_ref as V
from test_features_gpu import u32

pytestmark = pytest.mark.gpu


def scene_of(ctx, k):
    sc = gsrt.Scene.from_params(ctx, k.params, k.aabbs)
    sc.build_bvh()
    return sc


def hold_radii(k, got, x64, valid):
    """got against the float64 reference, with the band's allowance of 1"""
    store = k.seen & valid
    assert np.array_equal(u32(got)[~store], u32(k.radii)[~store])  # unseen, behind the camera, singular: every bit kept
    band = V.in_band(x64) & store
    assert band.sum() <= 0.02 * max(1, store.sum())
    r = np.ceil(x64)
    ok = np.zeros(k.n, bool)
    for shift, where in ((0.0, store), (-1.0, band), (1.0, band)):
        with np.errstate(invalid="ignore"):
            want = V.radii_after((r + shift).astype(np.float32), valid, k.seen, k.radii)
        ok |= where & (u32(got) == u32(want))
    assert ok[store].all(), np.nonzero(store & ~ok)[0][:8]
    return int(store.sum()), int(band.sum())


@pytest.mark.parametrize("n", V.SIZES)
def test_stats_and_radii(ctx, n):
    import torch

    k, ubo = V.case(n), V.camera()
    x64, valid = V.radius_f64(ubo, k.params)
    want_stats = gsrt.density_stats_add(ctx, k.rows, k.stats.copy(), V.WIDTH, V.HEIGHT)
    twice = gsrt.density_stats_add(ctx, k.rows, want_stats.copy(), V.WIDTH, V.HEIGHT)
    sc = scene_of(ctx, k)
    try:
        # host arrays
        stats, radii = k.stats.copy(), k.radii.copy()
        out = gsrt.view_stats_add(sc, ubo, k.rows, stats, radii)
        assert out[0] is stats and out[1] is radii
        assert np.array_equal(u32(stats), u32(want_stats))
        assert np.array_equal(u32(stats)[~k.seen], u32(k.stats)[~k.seen])
        stored, in_band = hold_radii(k, radii, x64, valid)
        print(f"n = {n}: {stored} radii stored, {in_band} in the band")
        if n > 1:
            grew = k.seen & valid & (u32(k.radii) == 0)
            assert grew.sum() > n // 8 and (radii[grew] >= 1).all() and (u32(radii) != u32(k.radii)).sum() == grew.sum()
        # again: the statistic accumulates, the maximum stays
        again = radii.copy()
        sc.view_stats_add(ubo, k.rows, stats, again)
        assert np.array_equal(u32(stats), u32(twice)) and np.array_equal(u32(again), u32(radii))
        # without radii: the statistic alone
        alone = k.stats.copy()
        gsrt.view_stats_add(sc, ubo, k.rows, alone)
        assert np.array_equal(u32(alone), u32(want_stats))
        # device arrays, blocking and enqueued: the host form's bits
        for asynchronous in (False, True):
            d_rows, d_stats, d_radii = (torch.from_numpy(a.copy()).to("cuda:0") for a in (k.rows, k.stats, k.radii))
            torch.cuda.synchronize()
            gsrt.view_stats_add(sc, ubo, d_rows.data_ptr(), d_stats.data_ptr(), d_radii.data_ptr(), asynchronous=asynchronous)
            ctx.synchronize()
            assert np.array_equal(u32(d_stats.cpu().numpy()), u32(want_stats))
            assert np.array_equal(u32(d_radii.cpu().numpy()), u32(radii))
    finally:
        sc.close()


def test_refusals(ctx):
    import torch

    k, ubo = V.case(257), V.camera()
    L = gsrt.lib
    stats, radii = k.stats.copy(), k.radii.copy()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    assert L.gsrt_view_stats_add(None, p(ubo), p(k.rows), p(stats), p(radii)) == gsrt.E_ARG
    sc = gsrt.Scene.from_params(ctx, k.params, k.aabbs)
    try:
        assert L.gsrt_view_stats_add(sc.handle, p(ubo), p(k.rows), p(stats), p(radii)) == gsrt.E_STATE  # no BVH yet
        assert "gsrt_build_bvh" in L.gsrt_last_error(ctx.handle).decode()
        sc.build_bvh()
        assert L.gsrt_view_stats_add(sc.handle, None, p(k.rows), p(stats), p(radii)) == gsrt.E_ARG
        assert L.gsrt_view_stats_add(sc.handle, p(ubo), None, p(stats), p(radii)) == gsrt.E_ARG
        assert L.gsrt_view_stats_add(sc.handle, p(ubo), p(k.rows), None, p(radii)) == gsrt.E_ARG
        for field in ("width", "height"):
            empty = ubo.copy()
            empty[field] = 0
            assert L.gsrt_view_stats_add(sc.handle, p(empty), p(k.rows), p(stats), p(radii)) == gsrt.E_ARG
        d_radii = torch.zeros(257, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        assert L.gsrt_view_stats_add(sc.handle, p(ubo), p(k.rows), p(stats), ctypes.c_void_p(d_radii.data_ptr())) == gsrt.E_ARG
        assert "all be" in L.gsrt_last_error(ctx.handle).decode()
        assert L.gsrt_view_stats_add_async(sc.handle, p(ubo), None, None, None) == gsrt.E_ARG
        assert np.array_equal(u32(stats), u32(k.stats)) and np.array_equal(u32(radii), u32(k.radii))  # nothing was written
        sc.add_mesh(*gsrt.sphere_mesh((0.0, 0.0, -3.0), 0.5))
        assert L.gsrt_view_stats_add(sc.handle, p(ubo), p(k.rows), p(stats), p(radii)) == gsrt.E_ARG
        assert "mesh" in L.gsrt_last_error(ctx.handle).decode()
    finally:
        sc.close()
