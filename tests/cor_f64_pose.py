"""The float64 backward of a COR frame to the camera's model-view matrix -- test infrastructure beside
tests/cor_f64_geom.py, whose project() it imports (the projection is not restated here).

  pose_chain:  the splat rows (dL/d(ppx, ppy, A, B, C) in slots 0..4, dL/d(view depth) in slot 6 for the depth form) back
               through the projection to the 16 entries of MV, with MV's inverse (the rays) held fixed: include/gsrt.h,
               gsrt_pose_grad. The chain is cor_f64_geom._chain's up to the view-space position t = MV (c, 1) and the
               Jacobian rows T = J MV_3x3, written out again because that one returns only what follows them.
  twist, apply_twist, log_twist: the tangent space of a left perturbation MV' = exp(xi^) MV, xi = (v, w).

Everything is numpy float64. Matrices are ordinary (4, 4) arrays M[r, c]; the ubo's arrays hold entry [r, c] at c * 4 + r.
"""
import numpy as np

import cor_f64 as F
import cor_f64_geom as Q

FAULTS = ("direct", "transpose", "slot6", "bottom")


def _pose(p, center, rows, depth, absolute, fault=None):
    """(n, 4, 4): each Gaussian's dL/dMV[r, c]. absolute: every factor by its absolute value and every difference as a sum,
    i.e. the sum of the absolute values of the products the chain forms. fault: one of FAULTS, a chain with that mistake
    (tests/test_pose_ref.py shows that the GPU test's bound sees each of them)."""
    ab = np.abs if absolute else (lambda x: x)
    sgn = 1.0 if absolute else -1.0
    u = p.u
    MV, P = ab(u.MV), ab(u.P)
    rows = ab(np.asarray(rows, np.float64))
    gpx, gpy, gA, gB, gC = (rows[:, k] for k in range(5))
    n = p.n
    Qm = ab(np.stack([np.stack([p.A, p.B], -1), np.stack([p.B, p.C], -1)], -2))
    G = np.stack([np.stack([gA, gB / 2], -1), np.stack([gB / 2, gC], -1)], -2)
    W = sgn * (Qm @ G @ Qm)  # dL/dV = -Q G Q
    T, S = ab(p.T), ab(p.S)
    gT = 2.0 * (W @ (T @ S))  # (n, 2, 3): dL/dT0, dL/dT1
    gj00, gj02 = gT[:, 0] @ MV[0, :3], gT[:, 0] @ MV[2, :3]
    gj11, gj12 = gT[:, 1] @ MV[1, :3], gT[:, 1] @ MV[2, :3]
    t, idd = ab(p.t), ab(p.id)
    fx, fy = (abs(p.fx), abs(p.fy)) if absolute else (p.fx, p.fy)
    gid = gj00 * fx + gj11 * fy + 2.0 * idd * (gj02 * fx * t[:, 0] + gj12 * fy * t[:, 1])
    gt = np.zeros((n, 4))
    gt[:, 0] = gj02 * fx * idd ** 2
    gt[:, 1] = gj12 * fy * idd ** 2
    gt[:, 2] = gid * idd ** 2
    ph = ab(p.ph)
    iw = 1.0 / np.where(p.valid, ph[:, 3], 1.0)
    gnx, gny = gpx * u.W / 2.0, gpy * u.H / 2.0
    gph = np.zeros((n, 4))
    gph[:, 0], gph[:, 1] = gnx * iw, gny * iw
    gph[:, 3] = sgn * (gnx * ph[:, 0] + gny * ph[:, 1]) * iw * iw
    gt = gt + gph @ P
    if depth and fault != "slot6":
        gt[:, 2] += sgn * rows[:, 6]  # the view depth is -t2
    c4 = ab(np.concatenate([np.asarray(center, np.float64), np.ones((n, 1))], 1))
    out = gt[:, :, None] * c4[:, None, :]  # t_r = sum_c MV[r, c] c4[c]
    if fault != "direct":
        # T0 = j02 MVz + j00 MVx, T1 = j12 MVz + j11 MVy: rows 0, 1 and 2 of MV's 3x3 stand in T themselves
        j00, j02 = fx * idd, fx * t[:, 0] * idd ** 2
        j11, j12 = fy * idd, fy * t[:, 1] * idd ** 2
        out[:, 0, :3] += gT[:, 0] * j00[:, None]
        out[:, 1, :3] += gT[:, 1] * j11[:, None]
        out[:, 2, :3] += gT[:, 0] * j02[:, None] + gT[:, 1] * j12[:, None]
    if fault == "bottom":
        out[:, 3, :] = 0.0
    if fault == "transpose":
        out = np.transpose(out, (0, 2, 1))
    out[~p.valid] = 0.0
    return out


class PoseChain:
    """What pose_chain returns: G (4, 4) = dL/dMV, M (4, 4) the same chain on absolute values, Mg (n, 4, 4) its per-Gaussian
    form (M = Mg.sum(0)), kappa (n,), valid (n,)"""


def pose_chain(ubo, center, cov, rows, depth=False, fault=None):
    """rows (n, >= 5; >= 7 with depth) to dL/dMV in float64, MV's inverse held fixed. Invalid splats (depth <= 0 or
    det <= 0) contribute nothing. kappa = v00 v11 / det as cor_f64_geom.model_chain's."""
    p = Q.project(ubo, center, cov)
    out = PoseChain()
    out.G = _pose(p, center, rows, depth, False, fault).sum(0)
    out.Mg = _pose(p, center, rows, depth, True)
    out.M = out.Mg.sum(0)
    out.valid = p.valid
    out.kappa = np.where(p.valid, p.V[:, 0, 0] * p.V[:, 1, 1] / np.where(p.valid, p.det, 1.0), 0.0)
    return out


def bound(ref, n_ops, eps=2.0 ** -24):
    """The GPU test's bound per entry of G: sum_g N (1 + kappa_g) eps Mg + eps |G| (every one of the kernel's N rounded
    operations rounds a value Mg bounds, the recomputed conic carries kappa_g, and the double sum is rounded to float once)"""
    return (n_ops * (1.0 + ref.kappa)[:, None, None] * eps * ref.Mg).sum(0) + eps * np.abs(ref.G)


def mat(a16):
    """(4, 4) M[r, c] from a ubo array of 16"""
    return np.asarray(a16, np.float64).reshape(4, 4).T


def twist(MV, G):
    """(dL/dv, dL/dw) of MV' = exp(xi^) MV at xi = 0: dL = <G, xi^ MV> = <G MV^T, xi^>"""
    H = np.asarray(G, np.float64) @ np.asarray(MV, np.float64).T
    return np.array([H[0, 3], H[1, 3], H[2, 3], H[2, 1] - H[1, 2], H[0, 2] - H[2, 0], H[1, 0] - H[0, 1]])


def hat(xi):
    v, w = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    X = np.zeros((4, 4))
    X[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    X[:3, 3] = v
    return X


def expm(X):
    """exp of a 4x4 by scaling and squaring of its Taylor series (|X| up to a few units: |w| = pi)"""
    X = np.asarray(X, np.float64)
    s = max(0, int(np.ceil(np.log2(max(np.abs(X).sum(1).max(), 1e-300)))) + 4)
    A = X / 2.0 ** s
    E, term = np.eye(4), np.eye(4)
    for k in range(1, 20):
        term = term @ A / k
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


def apply_twist(MV, MVinv, xi):
    """(exp(xi^) MV, MVinv exp(-xi^))"""
    return expm(hat(xi)) @ np.asarray(MV, np.float64), np.asarray(MVinv, np.float64) @ expm(-hat(np.asarray(xi, np.float64)))


def log_twist(E):
    """xi with exp(xi^) = E for a rigid E near the identity (|w| < pi): the pose error of the refinement test"""
    E = np.asarray(E, np.float64)
    R, t = E[:3, :3], E[:3, 3]
    th = np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    w = a if th < 1e-8 else a * th / np.sin(th)
    K = hat(np.concatenate([np.zeros(3), w]))[:3, :3]
    if th < 1e-8:
        Vinv = np.eye(3) - 0.5 * K
    else:
        Vinv = np.eye(3) - 0.5 * K + (1.0 / th ** 2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))) * (K @ K)
    return np.concatenate([Vinv @ t, w])


def linear_functional(ubo, MV, center, cov, rows, depth=False):
    """sum_g rows_g . (ppx, ppy, A, B, C[, depth])(MV) over the Gaussians valid at the ubo's own MV, through
    cor_f64_geom.project with only MV replaced: what pose_chain differentiates"""
    u = F.Ubo(ubo)
    valid = Q.project(u, center, cov).valid
    u.MV = np.asarray(MV, np.float64)
    p = Q.project(u, center, cov)
    rows = np.asarray(rows, np.float64)
    vals = np.stack([p.ppx, p.ppy, p.A, p.B, p.C], -1)
    s = (rows[:, :5] * vals)[valid].sum()
    if depth:
        s += (rows[:, 6] * p.depth)[valid].sum()
    return s
