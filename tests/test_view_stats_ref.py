"""tests/view_stats_ref.py on the CPU: the float32 restatement of the screen radius against the float64 one, the band
tests/test_view_stats_gpu.py uses, and the inputs.

Measured over the seen valid Gaussians of the three cases (764): the largest relative difference between radius_f32 and
radius_f64 is 4.95e-7 (view_stats_ref.MEASURED_REL = 5e-7 holds it), so the band is 8 x 5e-7 = 4e-6 relative to x; none
of the 764 float64 values lies that close to an integer (the limit is 2 %)."""
import numpy as np

import gsrt
import view_stats_ref as V


def test_f32_restatement_against_f64():
    worst, xs = V.measured()
    print(f"radius_f32 against radius_f64: worst relative difference {worst:.3g} over {xs.size} Gaussians")
    assert xs.size > 700
    assert V.MEASURED_REL / 2 < worst <= V.MEASURED_REL  # the recorded figure is the measurement, rounded up
    assert V.BAND == 8 * V.MEASURED_REL


def test_the_reference_alone_stays_out_of_the_band():
    _, xs = V.measured()
    share = float(V.in_band(xs).mean())
    print(f"share of float64 radii within {V.BAND:.3g} (relative) of an integer: {share:.4f}")
    assert share <= 0.02


def test_ceil_agrees_outside_the_band():
    ubo = V.camera()
    for n in V.SIZES:
        k = V.case(n)
        x64, valid = V.radius_f64(ubo, k.params)
        x32, _ = V.radius_f32(ubo, k.params)
        use = valid & k.seen & ~V.in_band(x64)
        assert np.array_equal(np.ceil(x32[use]).astype(np.float64), np.ceil(x64[use]))


def test_radius_of_a_centred_isotropic_gaussian():
    """on the optical axis at depth d an isotropic Gaussian of scale s has V = ((f s / d)^2 + 0.3) I with f = P00 W / 2
    (= P11 H / 2 for square pixels), a zero discriminant held at 0.1, and x = 3 sqrt(V00 + sqrt(0.1))"""
    W = H = 64
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 1, 16)
    f = 0.5 * H / np.tan(np.radians(30.0))
    params = np.zeros((3, 12), np.float32)
    for i, (s, d) in enumerate(((0.1, 2.0), (0.5, 4.0), (0.02, 1.0))):
        params[i, 2], params[i, 3] = -d, 0.5
        params[i, [4, 7, 9]] = s * s
        want = 3.0 * np.sqrt((f * s / d) ** 2 + 0.3 + np.sqrt(0.1))
        x64, valid = V.radius_f64(ubo, params[i:i + 1])
        x32, _ = V.radius_f32(ubo, params[i:i + 1])
        assert valid[0] and abs(x64[0] - want) <= 1e-5 * want and abs(float(x32[0]) - want) <= 1e-5 * want


def test_inputs():
    ubo = V.camera()
    for n in V.SIZES:
        k = V.case(n)
        x64, valid = V.radius_f64(ubo, k.params)
        assert k.seen[0] and (n == 1 or 0.25 < (~k.rows.any(1)).mean() < 0.42)  # about a third all +0
        if n == 1:
            assert valid[0]
            continue
        u = k.rows.view(np.uint32)
        only_neg0 = (u[:, :6] == 0x80000000).any(1) & ~k.seen
        has_nan = np.isnan(k.rows[:, :6]).any(1)
        assert only_neg0.sum() >= 5 and (has_nan & k.seen).sum() >= 5
        assert not valid[[3, 5, 200]].any() and k.seen[[3, 5, 200]].all()  # behind, singular, behind: with non-zero rows
        pre = k.radii.view(np.uint32)
        assert (pre == 0).sum() > n // 4 and (k.radii == 1e4).sum() > n // 4 and (pre == 0x7FC00ABC).sum() > n // 12
        # the radii cover small and large splats; some lie above 3DGS's 20 px
        r = np.ceil(x64[valid & k.seen])
        assert r.min() <= 4 and (r > 20).sum() >= 5


def test_radii_after_keeps_nan_and_larger_words():
    x = np.array([5.2, 5.2, 5.2, np.nan, 7.0], np.float32)
    pre = np.array([0.0, 1e4, np.nan, 3.0, 0.0], np.float32)
    on = np.ones(5, bool)
    got = V.radii_after(x, on, on, pre)
    assert got[0] == 6 and got[1] == 1e4 and np.isnan(got[2]) and got[3] == 3 and got[4] == 7
    off = V.radii_after(x, np.zeros(5, bool), on, pre)
    assert off.view(np.uint32).tobytes() == pre.view(np.uint32).tobytes()
