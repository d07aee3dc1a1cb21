"""References for the optimiser step (gsrt_model_step and its neighbours), in numpy; not a test file.

adam_ref: the header's Adam with every operation rounded to float32 on its own (numpy's float32 arithmetic: no fused
multiply-add, correctly rounded square root and division), fed the scalars of gsrt.adam_scalars. step_ref applies it to a
whole model by group, with the frozen groups and the sparse rule.

activate_f64 / chain_f64: the activation and the chain to the raw parameters in float64, on tests/cor_f64_geom.py's
param_chain, with the magnitude sums (sums of absolute terms) the bounds of tests/test_model_step_gpu.py multiply.

The bounds' operation counts, in units of EPS = 2^-24 (half an ulp), a product counting one more than its factors together,
as gsrt_model_step.hip's chain_raw lists them. The ROCm documentation on the machine states no ulp bound for the device
expf and logf, so OpenCL full profile's is taken: 3 ulp each, E = 6 EPS; the library's divisions and square roots are
correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt): one EPS each.
"""
import numpy as np

import cor_f64_geom as Q
import test_grad_f64 as S

EPS = 2.0 ** -24
E_EXP = 6    # expf: 3 ulp (OpenCL full profile) = 6 EPS of the result
E_LOG = 6    # logf: 3 ulp = 6 EPS of the result
N_ACT = {"scale": E_EXP, "opacity": E_EXP + 2}   # s = expf(l); o: expf, 1 + e, the reciprocal
N_CHAIN = {"rot": 2 * E_EXP + 55, "scale": 2 * E_EXP + 38, "opacity": 2 * E_EXP + 7}
GROUPS = ("center", "rot", "scale", "opacity", "sh_dc", "sh_rest", "features")
f32 = np.float32


def adam_ref(p, m, v, g, beta1, beta2, eps, a1, a2, c2, ss):
    """(p', m', v') of float32 arrays p, m, v, g: m' = beta1 m + a1 g, v' = beta2 v + (a2 g) g,
    p' = p - (ss m') / (sqrt(v') / c2 + eps), every operation in float32"""
    p, m, v, g = (np.asarray(a, f32) for a in (p, m, v, g))
    beta1, beta2, eps, a1, a2, c2, ss = (f32(x) for x in (beta1, beta2, eps, a1, a2, c2, ss))
    with np.errstate(all="ignore"):
        m2 = beta1 * m + a1 * g
        v2 = beta2 * v + (a2 * g) * g
        p2 = p - (ss * m2) / (np.sqrt(v2) / c2 + eps)
    assert m2.dtype == v2.dtype == p2.dtype == f32
    return p2, m2, v2


def seen_rows(splat):
    """gsrt_density_stats_add's "seen": any of row[0..5] != 0.0f (a -0 is not seen, a NaN is)"""
    return (np.asarray(splat)[:, :6] != 0.0).any(axis=1)


def step_ref(raw, m, v, grad_geom, g_sh, g_feat, adam, scalars, seen):
    """The expected (raw', m', v') of gsrt_model_step: raw, m, v lists [center, rot, scale, opacity, sh or None, features or
    None]; grad_geom (n, 11) the chained gradient (centre 3, rot 4, log scale 3, logit 1); g_sh (n, 16, 3), g_feat (n, C) the
    tables; adam the gsrt.AdamParams, scalars gsrt.adam_scalars(adam); seen: the rows stepped (None: all)."""
    a1, a2, c2 = scalars[:3]
    ss = dict(zip(GROUPS, scalars[3:]))
    lr = {k: getattr(adam, "lr_" + k) for k in GROUPS}
    n = raw[0].shape[0]
    rows = np.ones(n, bool) if seen is None else np.asarray(seen, bool)
    out = [[None if a is None else a.copy() for a in t] for t in (raw, m, v)]

    def group(i, name, g, sel=Ellipsis):
        if lr[name] == 0.0:
            return
        p2, m2, v2 = adam_ref(raw[i][sel], m[i][sel], v[i][sel], g, adam.beta1, adam.beta2, adam.eps, a1, a2, c2, ss[name])
        for dst, new in zip(out, (p2, m2, v2)):
            view = dst[i][sel]
            view[rows] = new[rows]

    group(0, "center", grad_geom[:, 0:3])
    group(1, "rot", grad_geom[:, 3:7])
    group(2, "scale", grad_geom[:, 7:10])
    group(3, "opacity", grad_geom[:, 10])
    if raw[4] is not None:
        group(4, "sh_dc", g_sh[:, 0:1, :], (slice(None), slice(0, 1)))
        group(4, "sh_rest", g_sh[:, 1:, :], (slice(None), slice(1, None)))
    if raw[5] is not None:
        group(5, "features", g_feat)
    return out


def normalise_f32(rot):
    """(nq, q) of gsrt.h's activation in float32: nq = sqrt(((r r + x x) + y y) + z z), q = rot / nq, rot where nq == 0"""
    r = np.asarray(rot, f32)
    nq = np.sqrt(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]) + r[:, 3] * r[:, 3])
    with np.errstate(all="ignore"):
        q = np.where(nq[:, None] == 0, r, r / nq[:, None])
    assert nq.dtype == f32 and q.dtype == f32
    return nq, q


class Act:
    """activate_f64's result: nq (n,), q (n, 4), s (n, 3), o (n,) in float64"""


def activate_f64(rot, log_scale, logit):
    a = Act()
    r = np.asarray(rot, np.float64)
    a.nq = np.sqrt((r * r).sum(1))
    a.q = np.where(a.nq[:, None] == 0, r, r / np.where(a.nq == 0, 1.0, a.nq)[:, None])
    a.s = np.exp(np.asarray(log_scale, np.float64))
    with np.errstate(over="ignore"):
        a.o = 1.0 / (1.0 + np.exp(-np.asarray(logit, np.float64)))
    return a


class Chain:
    """chain_f64's result: rot (n, 4), scale (n, 3) (log scale's), opacity (n,) (the logit's) and M_rot, M_scale, M_opacity"""


def chain_f64(rot, log_scale, logit, dcov, dop):
    """dL/d(raw rot, log scale, logit) from dcov (n, 6) = dL/d(cov3d) and dop (n,) = dL/d(opacity) in float64:
    param_chain at q = rot / |rot| and s = exp(log scale), then d log_scale = d s * s, d raw_rot = (dq - q (q . dq)) / |rot|
    (0 at the zero quaternion), d logit = dop o (1 - o). The M's are the same sums with every term by its absolute value
    (1 - o counts as 1 + o)."""
    a = activate_f64(rot, log_scale, logit)
    d64 = np.asarray(dcov, np.float64)
    pc = Q.param_chain(a.q, a.s, d64, np.abs(d64))
    c = Chain()
    c.scale, c.M_scale = pc.scale * a.s, pc.M_scale * a.s
    zero = a.nq == 0
    inv = np.where(zero, 0.0, 1.0 / np.where(zero, 1.0, a.nq))[:, None]
    qd = (a.q * pc.rot).sum(1, keepdims=True)
    mqd = (np.abs(a.q) * pc.M_rot).sum(1, keepdims=True)
    c.rot = (pc.rot - a.q * qd) * inv
    c.M_rot = (pc.M_rot + np.abs(a.q) * mqd) * inv
    dop = np.asarray(dop, np.float64)
    c.opacity, c.M_opacity = dop * a.o * (1.0 - a.o), np.abs(dop) * a.o * (1.0 + a.o)
    return c


class Case:
    """case()'s result: raw, m, v (lists of six), grads (center, cov, splat, sh, features), the special rows' indices"""

    def adam(self, gsrt, step=1, sparse=False):
        """the rates of the case: every group moves except log scale (lr 0: the frozen group)"""
        return gsrt.adam_params(lr_center=1e-3, lr_rot=2e-3, lr_scale=0.0, lr_opacity=5e-2, lr_sh_dc=2.5e-3,
                                lr_sh_rest=1.25e-4, lr_features=1e-2, step=step, sparse=sparse)

    def copies(self):
        return [[None if a is None else a.copy() for a in t] for t in (self.raw, self.m, self.v)]


_CASES = {}


def case(n, seed=5, with_sh=True, channels=0):
    """A raw model of n Gaussians cut from or tiled out of test_grad_f64.scene() (300): raw = log / logit of it (opacities
    capped at 0.99, so that every logit is finite), each quaternion scaled by a random factor in [0.5, 2]; random moments
    with v >= 0; random gradient tables; about a third of the splat rows +0 in slots 0..5 (slot 6 set, which must not
    count); and, from n = 8 on, row 1 all -0 (not seen), row 2 a NaN in slot 0 and +0 otherwise (seen), row 3 the zero
    quaternion. The frozen group is Case.adam's lr_scale = 0. Cached: treat the arrays as read-only (Case.copies)."""
    key = (n, seed, with_sh, channels)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(seed + 1000 * n + channels)
    c0, r0, s0, o0, sh0 = S.scene()
    idx = np.arange(n) % S.N
    tile = (np.arange(n) // S.N).astype(f32)[:, None]
    k = Case()
    k.n = n
    center = (c0[idx] + f32(0.01) * tile).astype(f32)
    rot = (r0[idx] * rng.uniform(0.5, 2.0, (n, 1))).astype(f32)
    log_scale = np.log(s0[idx].astype(np.float64)).astype(f32)
    o = np.minimum(o0[idx].astype(np.float64), 0.99)
    logit = np.log(o / (1.0 - o)).astype(f32)
    sh = np.ascontiguousarray(sh0[idx]) if with_sh else None
    feat = rng.uniform(-1, 1, (n, channels)).astype(f32) if channels else None
    k.special = n >= 8
    if k.special:
        k.neg0_row, k.nan_row, k.zero_quat = 1, 2, 3
        rot[k.zero_quat] = 0.0
    k.raw = [center, rot, log_scale, logit, sh, feat]
    k.m = [None if a is None else (rng.normal(0, 0.05, a.shape)).astype(f32) for a in k.raw]
    k.v = [None if a is None else (rng.uniform(0, 0.01, a.shape)).astype(f32) for a in k.raw]
    splat = rng.uniform(-1, 1, (n, 8)).astype(f32)
    splat[:, 7] = 0.0
    unseen = rng.random(n) < 1.0 / 3.0
    splat[unseen, :6] = 0.0
    if k.special:
        splat[k.neg0_row, :6] = -0.0
        splat[k.nan_row, :6] = 0.0
        splat[k.nan_row, 0] = np.nan
    k.grads = [rng.uniform(-1, 1, (n, 3)).astype(f32), rng.uniform(-1, 1, (n, 6)).astype(f32), splat,
               rng.uniform(-1, 1, (n, 16, 3)).astype(f32) if with_sh else None,
               rng.uniform(-1, 1, (n, channels)).astype(f32) if channels else None]
    k.seen = seen_rows(splat)
    _CASES[key] = k
    return k
