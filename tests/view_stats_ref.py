"""The screen radius of gsrt_view_stats_add (include/gsrt.h) on the CPU, twice, and the inputs its tests share.

  radius_f64:  float64. V = T Sigma T^T + 0.3 I is cor_f64_geom.project's (imported, not copied: its own formulas, no
               operation order shared with the kernels); the radius from it: lam = the larger eigenvalue of V with the
               discriminant held at >= 0.1, x = 3 sqrt(lam). The library stores ceil(x).
  radius_f32:  numpy float32, every operation rounded on its own in the order gsrt_project.hpp's cor_chain and the header
               write them; an fmaf is the exact product and sum in float64 rounded to float32 (a float32 product is exact in
               float64; the sum is rounded twice, which can differ from a true fmaf in the last bit and stays within the
               measured difference below).

tests/test_view_stats_ref.py holds the two to each other and fixes the band tests/test_view_stats_gpu.py uses."""
import numpy as np

import cor_f64 as F64
import cor_f64_geom as Q
import gsrt

F = np.float32
SIZES = (1, 257, 1000)
WIDTH, HEIGHT = 160, 96
SEED = 11
_CACHE = {}


def camera():
    return gsrt.camera_from_modelview(gsrt.lookat((0.3, -0.2, 0.5), (0.1, 0.0, -4.0)), 55.0, WIDTH, HEIGHT, 1.0, 1, 16)


def radius_f64(ubo, params):
    """(x = 3 sqrt(lam) in float64, valid) for gsrt_gauss_param rows (n, 12) as float32 holds them"""
    p = np.asarray(params, F).astype(np.float64)
    with np.errstate(all="ignore"):
        pr = Q.project(ubo, p[:, :3], p[:, 4:10])
        mid = 0.5 * (pr.V[:, 0, 0] + pr.V[:, 1, 1])
        disc = mid * mid - pr.det
        lam = mid + np.sqrt(np.fmax(0.1, disc))
        x = 3.0 * np.sqrt(lam)
    return x, pr.valid


def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


def radius_f32(ubo, params):
    """(x = 3.0f * sqrtf(lam) before the ceilf, valid): cor_chain and the header's five lines in float32"""
    u = ubo.reshape(-1)[0] if ubo.dtype.names else ubo
    MV, P = np.asarray(u["model_view"], F).reshape(16), np.asarray(u["projection"], F).reshape(16)
    cm = lambda m, c, r: m[c * 4 + r]  # noqa: E731
    g = np.asarray(params, F)
    c4 = [g[:, 0], g[:, 1], g[:, 2], np.ones(len(g), F)]
    with np.errstate(all="ignore"):
        t = [((cm(MV, 0, r) * c4[0] + cm(MV, 1, r) * c4[1]) + cm(MV, 2, r) * c4[2]) + cm(MV, 3, r) * c4[3] for r in range(4)]
        depth = -t[2]
        front = depth > F(0.0)
        fx = (cm(P, 0, 0) * F(u["width"])) * F(0.5)
        fy = (cm(P, 1, 1) * F(u["height"])) * F(0.5)
        idep = F(1.0) / depth
        id2 = idep * idep
        j00, j02, j11, j12 = fx * idep, (fx * t[0]) * id2, fy * idep, (fy * t[1]) * id2
        T0 = [_fma(j02, np.full_like(j02, cm(MV, k, 2)), j00 * cm(MV, k, 0)) for k in range(3)]
        T1 = [_fma(j12, np.full_like(j12, cm(MV, k, 2)), j11 * cm(MV, k, 1)) for k in range(3)]
        cv = [g[:, 4 + k] for k in range(6)]
        Sg = [[cv[0], cv[1], cv[2]], [cv[1], cv[3], cv[4]], [cv[2], cv[4], cv[5]]]
        dot3 = lambda a, b: _fma(a[2], b[2], _fma(a[1], b[1], a[0] * b[0]))  # noqa: E731
        u0 = [dot3(Sg[r], T0) for r in range(3)]
        u1 = [dot3(Sg[r], T1) for r in range(3)]
        v00 = dot3(T0, u0) + F(0.3)
        v01 = dot3(T0, u1)
        v11 = dot3(T1, u1) + F(0.3)
        det = _fma(v00, v11, -(v01 * v01))
        valid = front & (det > F(0.0))
        mid = F(0.5) * (v00 + v11)
        disc = _fma(mid, mid, -det)
        lam = mid + np.sqrt(np.fmax(F(0.1), disc))
        x = F(3.0) * np.sqrt(lam)
    assert x.dtype == F
    return x, valid


def radii_after(x32, valid, seen, radii):
    """radii after the call, from the float32 x: r = ceilf(x); if (r > radii[g]) radii[g] = r, for seen valid Gaussians"""
    out = np.array(radii, F, copy=True)
    with np.errstate(all="ignore"):
        r = np.ceil(x32)
        store = seen & valid & (r > out)
    out[store] = r[store]
    return out


def case(n):
    """The inputs of size n, made once and not changed: a namespace of
      params (n, 12), aabbs (n, 6): a synthetic model in front of camera(); from n >= 257 Gaussians 3 and 200 lie behind
          the camera and Gaussian 5 has a NaN in cov3d (singular), all three with non-zero rows;
      rows (n, 8): about a third all +0; every 11th of the others only a -0 (not seen), every 13th a NaN in slot 2 (seen);
      stats (n, 2), radii (n,): the arrays before the call; radii a mix of +0, 1e4 and a NaN pattern;
      seen (n,) bool."""
    if n in _CACHE:
        return _CACHE[n]
    from types import SimpleNamespace

    rng = np.random.default_rng(SEED + n)
    center = np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(-2.0, 2.0, n), rng.uniform(-9.0, -1.5, n)], 1).astype(F)
    rot = rng.normal(size=(n, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(F)
    scale = np.exp(rng.uniform(np.log(0.005), np.log(0.6), (n, 3))).astype(F)
    cov = Q.cov6(F64.covariance(rot, scale)).astype(F)
    if n >= 257:
        center[3, 2], center[200, 2] = F(4.0), F(0.6)  # behind the camera (the eye is at z = 0.5 looking down -z)
        cov[5, 0] = np.nan
    params = np.zeros((n, 12), F)
    params[:, :3], params[:, 3], params[:, 4:10] = center, F(0.5), cov
    ext = (3.0 * scale.max(1))[:, None]
    aabbs = np.concatenate([center - ext, center + ext], 1).astype(F)
    rows = rng.normal(0.0, 1e-3, (n, 8)).astype(F)
    kind = rng.integers(0, 3, n)
    kind[0] = 1  # the only Gaussian of n = 1 is seen
    rows[kind == 0] = F(0.0)
    others = np.nonzero(kind != 0)[0]
    rows[others[1::11], :] = F(0.0)
    rows[others[1::11], 4] = F(-0.0)
    rows[others[1::11], 6:] = F(1.0)  # slots 6 and 7 do not count
    rows[others[5::13], 2] = np.nan
    if n >= 257:
        rows[[3, 5, 200]] = F(2e-3)
    seen = (rows[:, :6] != 0).any(1)
    stats = rng.uniform(0.0, 3.0, (n, 2)).astype(F)
    stats[::5] = (-0.0, 0.0)
    stats.view(np.uint32)[3::7, 0] = 0x7FC01234
    radii = np.zeros(n, F)
    radii[1::3] = F(1e4)
    radii.view(np.uint32)[2::9] = 0x7FC00ABC
    _CACHE[n] = SimpleNamespace(n=n, params=params, aabbs=aabbs, rows=rows, stats=stats, radii=radii, seen=seen)
    return _CACHE[n]


def measured():
    """Over every seen valid Gaussian of every case: (the largest relative difference between radius_f32 and radius_f64,
    the share of them whose float64 x lies within BAND (relative) of an integer for that band)"""
    ubo = camera()
    worst, xs = 0.0, []
    for n in SIZES:
        k = case(n)
        x64, v64 = radius_f64(ubo, k.params)
        x32, v32 = radius_f32(ubo, k.params)
        assert np.array_equal(v64, v32)
        use = v64 & k.seen
        if use.any():
            worst = max(worst, float((np.abs(x32[use].astype(np.float64) - x64[use]) / x64[use]).max()))
            xs.append(x64[use])
    return worst, np.concatenate(xs)


# The band of tests/test_view_stats_gpu.py: 8 x the largest relative difference test_view_stats_ref.py measures between
# the two restatements over these cases (see MEASURED_REL there; the test fails when the measurement leaves it).
MEASURED_REL = 5e-7
BAND = 8 * MEASURED_REL


def in_band(x64, band=None):
    band = BAND if band is None else band
    return np.abs(x64 - np.rint(x64)) <= band * x64
