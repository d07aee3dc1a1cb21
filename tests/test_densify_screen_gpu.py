"""Densify with the screen-size prune (gsrt_densify_screen, gsrt_densify_screen_async, gsrt_densify_screen_count) against
tests/densify_ref.py: the reference is run with the opacity of every radius-pruned Gaussian set to NaN, which the existing
rule (!(opacity >= min_opacity)) prunes, so model, origin and n_out must match bit for bit.

n in {1, 300, 1025} (one Gaussian, a second workgroup, five workgroups with one Gaussian in the last), with and without
SH. The radii are whole pixels in 1..60 against max_screen_radius = 20, with a NaN every 17th (does not prune) and the
bound itself every 19th (20 > 20 is false: kept)."""
import ctypes

import numpy as np
import pytest

import densify_ref as D
import gsrt
from test_densify_gpu import gpu_params, same_model, u32

pytestmark = pytest.mark.gpu

MAX_RADIUS = 20.0
SIZES = [1, 300, 1025]


def radii_of(n):
    r = np.random.default_rng(91 + n).integers(1, 61, n).astype(np.float32)
    r[3::17] = np.nan
    r[5::19] = np.float32(MAX_RADIUS)
    if n == 1:
        r[0] = 30.0
    return r


def reference(n, radii, max_radius):
    """densify_ref.densify with a NaN opacity where the radius prunes"""
    (c, r, s, o, sh, feat), stats, noise, P, plain = D.case(n)
    with np.errstate(invalid="ignore"):
        by_radius = (radii > np.float32(max_radius)) if max_radius > 0 else np.zeros(n, bool)
    o2 = o.copy()
    o2[by_radius] = np.nan
    return D.densify(c, r, s, o2, sh, feat, stats, noise, P), plain, by_radius


@pytest.mark.parametrize("with_sh", [False, True], ids=["nosh", "sh"])
@pytest.mark.parametrize("n", SIZES)
def test_matches_the_reference(ctx, n, with_sh):
    (c, r, s, o, sh, feat), stats, noise, P, _ = D.case(n)
    radii = radii_of(n)
    ref, plain, by_radius = reference(n, radii, MAX_RADIUS)
    params = gpu_params(P)
    assert gsrt.densify_count(ctx, s, o, stats, params, radii=radii, max_screen_radius=MAX_RADIUS) == ref.n_out
    got = gsrt.densify(ctx, c, r, s, o, sh if with_sh else None, stats, noise, params, radii=radii,
                       max_screen_radius=MAX_RADIUS)
    assert got[0].shape[0] == ref.n_out
    same_model(got, ref, with_sh, False)
    if n == 1:
        assert ref.n_out == 0 and by_radius[0]
    else:
        # the term did something: Gaussians that the plain rule keeps or densifies are gone, and only those
        assert (by_radius & (plain.c > 0)).sum() >= 20 and ref.n_out < plain.n_out
        assert not np.isin(np.nonzero(by_radius)[0], np.where(got[6] >= 0, got[6], -1 - got[6])).any()
        kept = np.nonzero(~by_radius & (plain.c > 0))[0]
        assert np.isin(kept, np.where(got[6] >= 0, got[6], -1 - got[6])).all()
        nan_r = np.isnan(radii) & (plain.c > 0)
        at_bound = (radii == np.float32(MAX_RADIUS)) & (plain.c > 0)
        assert nan_r.sum() >= 5 and at_bound.sum() >= 5 and np.array_equal(ref.c[nan_r | at_bound], plain.c[nan_r | at_bound])


@pytest.mark.parametrize("n", SIZES)
def test_off_is_gsrt_densify(ctx, n):
    """radii=None, max_screen_radius = 0 and a negative one: gsrt.densify's bits (which equal the plain reference's)"""
    (c, r, s, o, sh, feat), stats, noise, P, plain = D.case(n)
    params, radii = gpu_params(P), radii_of(n)
    want = gsrt.densify(ctx, c, r, s, o, sh, stats, noise, params)
    same_model(want, plain, True, False)
    for kw in (dict(radii=None, max_screen_radius=MAX_RADIUS), dict(radii=radii, max_screen_radius=0.0),
               dict(radii=radii, max_screen_radius=-5.0)):
        got = gsrt.densify(ctx, c, r, s, o, sh, stats, noise, params, **kw)
        for a, b in zip(got, want):
            assert (a is None and b is None) or (a.shape == b.shape and a.tobytes() == b.tobytes())
        assert gsrt.densify_count(ctx, s, o, stats, params, **kw) == plain.n_out


def test_device_form_cap_and_refusals(ctx):
    import torch

    from gsrt.autograd import densify

    n = 1025
    (c, r, s, o, sh, feat), stats, noise, P, _ = D.case(n)
    radii = radii_of(n)
    ref, plain, _ = reference(n, radii, MAX_RADIUS)
    params = gpu_params(P)
    t = [torch.from_numpy(a).to("cuda:0") for a in (c, r, s, o, sh, stats, noise)]
    d_radii = torch.from_numpy(radii).to("cuda:0")
    got = densify(ctx, *t, params, radii=d_radii, max_screen_radius=MAX_RADIUS)  # gsrt_densify_screen_async
    same_model([g if g is None else g.cpu().numpy() for g in got], ref, True, False)
    assert gsrt.densify_count(ctx, t[2].data_ptr(), t[3].data_ptr(), t[5].data_ptr(), params, n=n,
                              radii=d_radii.data_ptr(), max_screen_radius=MAX_RADIUS) == ref.n_out
    # cap one row short: GSRT_E_ARG, n_out reported, nothing written
    cap = ref.n_out - 1
    out = [torch.full((cap, k), 123.0, dtype=torch.float32, device="cuda:0") for k in (3, 4, 3, 1, 48)]
    origin = torch.full((cap,), 77, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    a_in = gsrt.ModelArrays(*[x.data_ptr() for x in t[:5]], None, 0)
    a_out = gsrt.ModelArrays(*[x.data_ptr() for x in out], None, 0)
    n_out = ctypes.c_uint32(0)
    args = lambda radius: (ctx.handle, ctypes.byref(a_in), n, ctypes.c_void_p(t[5].data_ptr()),  # noqa: E731
                           ctypes.c_void_p(t[6].data_ptr()), ctypes.byref(params), ctypes.c_void_p(d_radii.data_ptr()),
                           ctypes.c_float(radius), ctypes.byref(a_out), ctypes.c_void_p(origin.data_ptr()), cap,
                           ctypes.byref(n_out))
    assert gsrt.lib.gsrt_densify_screen(*args(MAX_RADIUS)) == gsrt.E_ARG and n_out.value == ref.n_out
    assert str(ref.n_out) in gsrt.lib.gsrt_last_error(ctx.handle).decode()
    assert all(bool((x == 123.0).all()) for x in out) and bool((origin == 77).all())
    # a NaN bound, host radii among device arrays
    assert gsrt.lib.gsrt_densify_screen(*args(float("nan"))) == gsrt.E_ARG
    assert "max_screen_radius" in gsrt.lib.gsrt_last_error(ctx.handle).decode()
    with pytest.raises(gsrt.GsrtError) as e:
        gsrt.densify_count(ctx, s, o, stats, params, radii=radii, max_screen_radius=float("nan"))
    assert e.value.status == gsrt.E_ARG
    mixed = list(args(MAX_RADIUS))
    mixed[6] = ctypes.c_void_p(radii.ctypes.data)
    assert gsrt.lib.gsrt_densify_screen(*mixed) == gsrt.E_ARG and "all be" in gsrt.lib.gsrt_last_error(ctx.handle).decode()
    assert all(bool((x == 123.0).all()) for x in out)
