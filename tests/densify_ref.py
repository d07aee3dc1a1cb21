"""numpy reference of adaptive density control (include/gsrt.h: gsrt_density_stats_add, gsrt_densify_count, gsrt_densify)
and the inputs its tests share. float32 throughout, every operation rounded on its own, as the header writes them; the
decision is elementwise array arithmetic, the compaction a prefix sum and a plain loop over the Gaussians. It shares nothing
with the kernels: the rotation matrix is written out as gsrt.autograd.model_covariance writes it (row k, column j).

tests/test_densify_ref.py checks the reference and the inputs on the CPU; tests/test_densify_gpu.py holds the library to it
bit for bit."""
from types import SimpleNamespace

import numpy as np

import test_grad_f64 as S

F = np.float32
_CACHE = {}


def params(grad_threshold, split_scale, min_opacity, max_scale=0.0, shrink=1.6):
    return SimpleNamespace(grad_threshold=F(grad_threshold), split_scale=F(split_scale), min_opacity=F(min_opacity),
                           max_scale=F(max_scale), shrink=F(shrink))


def stats_add(rows, stats, width, height):
    """stats after one gsrt_density_stats_add of the (n, 8) rows: a new (n, 2) array"""
    rows = np.asarray(rows, F)
    out = np.array(stats, F, copy=True)
    hw, hh = F(0.5) * F(width), F(0.5) * F(height)
    with np.errstate(all="ignore"):
        for g in range(rows.shape[0]):
            row = rows[g]
            seen = False
            for k in range(6):
                if row[k] != F(0.0):  # a -0 compares equal, a NaN unequal
                    seen = True
            if seen:
                gx, gy = row[0] * hw, row[1] * hh
                norm = np.sqrt(gx * gx + gy * gy)
                out[g, 0] = out[g, 0] + norm
                out[g, 1] = out[g, 1] + F(1.0)
    return out


def decide(scale, opacity, stats, P):
    """(rows c in {0, 1, 2}, split, clone, prune by opacity, prune by scale) per Gaussian"""
    scale, opacity, stats = np.asarray(scale, F), np.asarray(opacity, F), np.asarray(stats, F)
    m = scale[:, 0].copy()
    m = np.where(scale[:, 1] > m, scale[:, 1], m)
    m = np.where(scale[:, 2] > m, scale[:, 2], m)
    with np.errstate(all="ignore"):
        mean = np.where(stats[:, 1] > F(0.0), stats[:, 0] / stats[:, 1], F(0.0)).astype(F)
        by_opacity = ~(opacity >= P.min_opacity)
        by_scale = (m > P.max_scale) if P.max_scale > F(0.0) else np.zeros(m.shape, bool)
        prune = by_opacity | by_scale
        dens = ~prune & (mean >= P.grad_threshold)
        split = dens & (m > P.split_scale)
    clone = dens & ~split
    c = np.where(prune, 0, np.where(dens, 2, 1)).astype(np.int64)
    return c, split, clone, by_opacity, by_scale


def rotation(rot):
    """R[k][j] (row k, column j) of gsrt.autograd.model_covariance, float32, as a 3 x 3 nest of (n,) arrays"""
    r, x, y, z = (np.asarray(rot, F)[:, i] for i in range(4))
    one, two = F(1.0), F(2.0)
    return [[one - two * (y * y + z * z), two * (x * y + r * z), two * (x * z - r * y)],
            [two * (x * y - r * z), one - two * (x * x + z * z), two * (y * z + r * x)],
            [two * (x * z + r * y), two * (y * z - r * x), one - two * (x * x + y * y)]]


def densify(center, rot, scale, opacity, sh, features, stats, noise, P):
    """The new model: a namespace of center, rot, scale, opacity, sh, features (None when absent), origin (int32), n_out
    and the per-Gaussian row counts c."""
    center, rot, scale, opacity = (np.asarray(a, F) for a in (center, rot, scale, opacity))
    noise = np.asarray(noise, F)
    n = center.shape[0]
    c, split, _, _, _ = decide(scale, opacity, stats, P)
    first = np.cumsum(c) - c  # o_g = the sum of c_h over h < g
    n_out = int(c.sum())
    src = np.zeros(n_out, np.int64)      # the Gaussian a row comes from
    child = np.full(n_out, -1, np.int64)  # 0 / 1: a split's child k; -1: a copy
    origin = np.zeros(n_out, np.int32)
    for g in range(n):
        o = int(first[g])
        if c[g] == 1:
            src[o], origin[o] = g, g
        elif c[g] == 2:
            src[o], src[o + 1] = g, g
            if split[g]:
                child[o], child[o + 1] = 0, 1
                origin[o], origin[o + 1] = -1 - g, -1 - g
            else:
                origin[o], origin[o + 1] = g, -1 - g
    out = SimpleNamespace(center=center[src].copy(), rot=rot[src].copy(), scale=scale[src].copy(), opacity=opacity[src].copy(),
                          sh=None if sh is None else np.asarray(sh, F)[src].copy(),
                          features=None if features is None else np.asarray(features, F)[src].copy(),
                          origin=origin, n_out=n_out, c=c)
    rows = np.nonzero(child >= 0)[0]
    if rows.size:
        g, k = src[rows], child[rows]
        R = rotation(rot[g])
        with np.errstate(all="ignore"):
            v = [scale[g, i] * noise[g, k, i] for i in range(3)]
            for j in range(3):
                x = (v[0] * R[0][j] + v[1] * R[1][j]) + v[2] * R[2][j]
                out.center[rows, j] = center[g, j] + x
            out.scale[rows] = scale[g] / P.shrink
    return out


# ---------------------------------------------------------------------------------------------- the tests' inputs
FEATURE_CHANNELS = 5


def model(n):
    """n Gaussians: the 300-Gaussian scene of tests/test_grad_f64.py repeated (Gaussian g is g mod 300 of it), with a
    5-channel feature table; from 300 on, a NaN opacity, a -0 and a NaN in the SH rows and a NaN feature, which a copy
    must keep bit for bit: (center, rot, scale, opacity, sh (n, 16, 3), features (n, 5))"""
    if n not in _CACHE:
        c, r, s, o, sh = S.scene()
        idx = np.arange(n) % S.N
        c, r, s, o, sh = (np.ascontiguousarray(a[idx]) for a in (c, r, s, o, sh))
        feat = np.random.default_rng(71).uniform(-4.0, 4.0, (n, FEATURE_CHANNELS)).astype(F)
        if n >= S.N:
            o[7] = np.nan
            sh[5, 0, 0], sh[6, 1, 1] = F(-0.0), np.nan
            feat[9, 2] = np.nan
        _CACHE[n] = (c, r, s, o, sh, feat)
    return _CACHE[n]


def synthetic_stats(n):
    """(n, 2) [sum, count]: counts 0..3, sums whose mean is uniform in [0, 1); and the (n, 2, 3) normal noise"""
    rng = np.random.default_rng(72)
    count = rng.integers(0, 4, n).astype(F)
    stats = np.stack([(rng.random(n).astype(F) * count).astype(F), count], 1)
    return np.ascontiguousarray(stats, F), rng.standard_normal((n, 2, 3)).astype(F)


def thresholds():
    """The rule every comparison uses, from quantiles of the 300-Gaussian model's own values: the mean gradient's median
    (0.5), the median largest scale for split against clone, the 10 % opacity, the 90 % largest scale."""
    _, _, s, o, _ = S.scene()
    m = s.max(axis=1)
    return params(0.5, np.quantile(m, 0.5), np.quantile(o, 0.1), np.quantile(m, 0.9), 1.6)


def case(n):
    """inputs and reference of size n, computed once: (model, stats, noise, params, reference with SH and features)"""
    key = ("case", n)
    if key not in _CACHE:
        mdl = model(n)
        stats, noise = synthetic_stats(n)
        P = thresholds()
        _CACHE[key] = (mdl, stats, noise, P, densify(*mdl, stats, noise, P))
    return _CACHE[key]
