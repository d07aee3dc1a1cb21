"""The float64 backward of a COR colour frame to the Gaussians' geometry -- test infrastructure beside tests/cor_f64.py.

Two steps, as the library takes them (include/gsrt.h, gsrt_render_splat_grad and gsrt_splat_grad_to_model):
  splat_gradients: L = <G, rgba> to each Gaussian's screen-space numbers, the pixel centre (ppx, ppy) and the conic (A, B, C)
                   of g = (A dx^2 + 2 B dx dy + C dy^2) / 2, dx = px - ppx, dy = py - ppy; it walks the hit lists of
                   cor_f64 (_tiles, _hits, _walk: imported, not copied) and forms dL/d alpha_i as cor_f64.gradients does;
  model_chain:     those five numbers back through the projection to the centre and the six cov3d entries.
And the step torch takes in gsrt.autograd.render_model, by hand:
  param_chain:     the six cov3d entries back to the rotation (a quaternion, used as given) and the scales.
project() restates the projection from (centre, cov3d) with its own formulas; a test holds it to cor_f64.Splats.

Everything is numpy float64. Nothing here shares a value or an operation order with the HIP kernels.
"""
import numpy as np

import cor_f64 as F

COV_IJ = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # cov3d[6] order: xx, xy, xz, yy, yz, zz


def cov6(S):
    """(n, 3, 3) symmetric -> (n, 6) in cov3d order"""
    S = np.asarray(S, np.float64)
    return np.stack([S[:, i, j] for i, j in COV_IJ], -1)


def cov33(c6):
    c6 = np.asarray(c6, np.float64)
    S = np.zeros((len(c6), 3, 3))
    for k, (i, j) in enumerate(COV_IJ):
        S[:, i, j] = S[:, j, i] = c6[:, k]
    return S


class Projection:
    """project()'s result: ppx, ppy, A, B, C, depth, valid (n,), and the intermediates model_chain needs"""


def project(ubo, center, cov):
    """The COR projection of (centre (n, 3), cov3d (n, 6) or (n, 3, 3)): depth = -view z, ppx = (ndc_x + 1) W / 2 with the
    general projection matrix, J the Jacobian of the pixel mapping at the view-space centre (fx = P00 W / 2, fy = P11 H / 2),
    T = J MV_3x3, V = T Sigma T^T + 0.3 I, (A, B, C) = V^-1. valid: depth > 0 and det V > 0."""
    u = ubo if isinstance(ubo, F.Ubo) else F.Ubo(ubo)
    c = np.asarray(center, np.float64)
    n = len(c)
    cov = np.asarray(cov, np.float64)
    S = cov33(cov) if cov.ndim == 2 else cov
    p = Projection()
    p.u, p.n, p.S = u, n, S
    p.t = np.concatenate([c, np.ones((n, 1))], 1) @ u.MV.T
    p.depth = -p.t[:, 2]
    front = p.depth > 0
    p.ph = p.t @ u.P.T
    w = np.where(front, p.ph[:, 3], 1.0)
    p.ppx = (p.ph[:, 0] / w + 1.0) * u.W / 2.0
    p.ppy = (p.ph[:, 1] / w + 1.0) * u.H / 2.0
    p.fx, p.fy = u.P[0, 0] * u.W / 2.0, u.P[1, 1] * u.H / 2.0
    p.id = 1.0 / np.where(front, p.depth, 1.0)
    J = np.zeros((n, 2, 3))
    J[:, 0, 0] = p.fx * p.id
    J[:, 0, 2] = p.fx * p.t[:, 0] * p.id ** 2
    J[:, 1, 1] = p.fy * p.id
    J[:, 1, 2] = p.fy * p.t[:, 1] * p.id ** 2
    p.T = J @ u.MV[:3, :3]
    p.V = p.T @ S @ np.transpose(p.T, (0, 2, 1)) + 0.3 * np.eye(2)
    p.det = p.V[:, 0, 0] * p.V[:, 1, 1] - p.V[:, 0, 1] * p.V[:, 1, 0]
    p.valid = front & (p.det > 0)
    d = np.where(p.valid, p.det, 1.0)
    p.A, p.B, p.C = p.V[:, 1, 1] / d, -p.V[:, 0, 1] / d, p.V[:, 0, 0] / d
    return p


class SplatGradients:
    """What splat_gradients returns: rows (n, 8), M (n, 8), near (rows, W) bool, digest (cor_f64.gradients' hash of the hit
    lists), opacity_M (n,) = M[:, 5]"""


def splat_gradients(ubo, center, rot, scale, opacity, sh=None, *, G_rgba, rows=None, tile=16, alpha_rel=1e-3,
                    trans_rel=1e-3, slab_rel=1e-5, depth_rel=1e-6, col_rel=1e-4):
    """The eight-slot rows of gsrt_render_splat_grad in float64. For a blended hit i of Gaussian g with o e_i < 0.99,
    dL/d alpha_i = d_i as cor_f64.gradients forms it (the colour behind the hit summed from the ray's last hit backwards),
    alpha_i = o e_i, so dL/dg_i = q_i = -alpha_i d_i, and g is a quadratic in (ppx, ppy, A, B, C):
        rows[g, 0] += q_i * -(A dx + B dy)    rows[g, 2] += q_i * dx^2 / 2    rows[g, 4] += q_i * dy^2 / 2
        rows[g, 1] += q_i * -(B dx + C dy)    rows[g, 3] += q_i * dx dy       rows[g, 5] += d_i * e_i
    A clamped hit adds nothing; slots 6 and 7 stay 0. The hits, their order, the slab test, the cuts and the stop are the
    forward's. M sums the absolute value of every product: with mag_i the sum of the absolute values of the terms of d_i
    (cor_f64.gradients' `mag`), |q_i| counts as alpha_i mag_i, slot 0 gets alpha_i mag_i (|A dx| + |B dy|), slots 2..4
    alpha_i mag_i times |dx^2 / 2|, |dx dy|, |dy^2 / 2|, and slot 5 mag_i e_i (cor_f64.gradients' M_opacity)."""
    import hashlib
    u = F.Ubo(ubo)
    sp = F.Splats(u, center, rot, scale, opacity, sh)
    n = sp.n
    r0, r1 = rows if rows else (0, u.H)
    near = np.zeros((u.H, u.W), bool)
    jit = F.jitter(u.seed, u.S)
    Gr = np.asarray(G_rgba, np.float64).reshape(u.H, u.W, 4) / u.S
    out = SplatGradients()
    out.rows, out.M = np.zeros((n, 8)), np.zeros((n, 8))
    digest = hashlib.sha256()
    for (ty, ye, tx, xe), cand, xs, ys in F._tiles(u, sp, r0, r1, tile):
        m = len(xs)
        tile_near = np.zeros(m, bool)
        iy, ix = ys.astype(np.int64), xs.astype(np.int64)
        for s, (jx, jy) in enumerate(jit):
            if not len(cand):
                continue
            px, py = xs + jx, ys + jy
            o, d = F.rays(u, px, py)
            h = F._hits(sp, cand, px, py, o, d, tile_near, alpha_rel, slab_rel, depth_rel)
            _, T_end, _ = F._walk(h, m, tile_near, trans_rel)
            F._clamps_near(sp, h, tile_near, alpha_rel, col_rel)
            b = h.blended
            r, g, a, Ti, col, e = h.ri[b], h.gi[b], h.alpha[b], h.T[b], h.col[b], h.e[b]
            is_open = h.oe[b] < 0.99
            digest.update(((iy[r] * u.W + ix[r]) * u.S + s).tobytes() + g.tobytes() + is_open.tobytes())
            w = a * Ti
            starts = np.searchsorted(r, np.arange(m))
            counts = np.bincount(r, minlength=m)
            S = np.zeros((len(r), 3))
            behind = np.zeros((m, 3))
            for k in range(int(counts.max()) - 1 if len(r) else -1, -1, -1):
                rr = np.nonzero(counts > k)[0]
                p = starts[rr] + k
                S[p] = behind[rr]
                behind[rr] += col[p] * w[p, None]
            Gs = Gr[iy[r], ix[r]]
            rinv = 1.0 / (1.0 - a)
            front, back = Ti[:, None] * col, S * rinv[:, None]
            tail = T_end[r] * rinv
            dLda = (Gs[:, :3] * (front - back)).sum(1) + Gs[:, 3] * tail
            mag = (np.abs(Gs[:, :3]) * (front + back)).sum(1) + np.abs(Gs[:, 3]) * tail
            dx, dy = px[r] - sp.ppx[g], py[r] - sp.ppy[g]
            A, B, C = sp.ca[g], sp.cb[g], sp.cc[g]
            q, qm = -a * dLda, a * mag
            terms = np.stack([q * -(A * dx + B * dy), q * -(B * dx + C * dy), q * 0.5 * dx * dx, q * dx * dy,
                              q * 0.5 * dy * dy, dLda * e, 0 * q, 0 * q], -1)
            mags = np.stack([qm * (np.abs(A * dx) + np.abs(B * dy)), qm * (np.abs(B * dx) + np.abs(C * dy)),
                             qm * 0.5 * dx * dx, qm * np.abs(dx * dy), qm * 0.5 * dy * dy, mag * e, 0 * q, 0 * q], -1)
            F._scatter(out.rows, g[is_open], terms[is_open])
            F._scatter(out.M, g[is_open], mags[is_open])
        near[ty:ye, tx:xe] = tile_near.reshape(ye - ty, xe - tx)
    out.near, out.digest = near[r0:r1], digest.hexdigest()
    return out


class ModelChain:
    """What model_chain returns: center (n, 3), cov (n, 6), M2_center, M2_cov (the same shapes), kappa (n,), valid (n,)"""


def _chain(p, rows, absolute):
    """dL/d(centre), dL/d(cov3d) from rows[:, :5] = dL/d(ppx, ppy, A, B, C). absolute: every factor by its absolute value
    and every difference as a sum, i.e. the sum of the absolute values of the products the chain forms."""
    ab = np.abs if absolute else (lambda x: x)
    sgn = 1.0 if absolute else -1.0
    u = p.u
    MV, P = ab(u.MV), ab(u.P)
    rows = ab(np.asarray(rows, np.float64))
    gpx, gpy, gA, gB, gC = (rows[:, k] for k in range(5))
    n = p.n
    Q = ab(np.stack([np.stack([p.A, p.B], -1), np.stack([p.B, p.C], -1)], -2))
    G = np.stack([np.stack([gA, gB / 2], -1), np.stack([gB / 2, gC], -1)], -2)
    W = sgn * (Q @ G @ Q)  # dL/dV = -Q G Q; the 0.3 I is a constant
    T, S = ab(p.T), ab(p.S)
    dS = np.transpose(T, (0, 2, 1)) @ W @ T  # dL/dSigma as a symmetric matrix
    cov = np.stack([dS[:, i, j] * (1.0 if i == j else 2.0) for i, j in COV_IJ], -1)  # an off-diagonal entry stands twice
    gT = 2.0 * (W @ (T @ S))  # (n, 2, 3)
    # T0 = j02 MVz + j00 MVx, T1 = j12 MVz + j11 MVy (rows 2, 0, 1 of MV's 3x3)
    gj00, gj02 = gT[:, 0] @ MV[0, :3], gT[:, 0] @ MV[2, :3]
    gj11, gj12 = gT[:, 1] @ MV[1, :3], gT[:, 1] @ MV[2, :3]
    t, idd, fx, fy = ab(p.t), ab(p.id), abs(p.fx) if absolute else p.fx, abs(p.fy) if absolute else p.fy
    # j00 = fx id, j02 = fx t0 id^2, j11 = fy id, j12 = fy t1 id^2, id = 1 / depth = -1 / t2
    gid = gj00 * fx + gj11 * fy + 2.0 * idd * (gj02 * fx * t[:, 0] + gj12 * fy * t[:, 1])
    gt = np.zeros((n, 4))
    gt[:, 0] = gj02 * fx * idd ** 2
    gt[:, 1] = gj12 * fy * idd ** 2
    gt[:, 2] = gid * idd ** 2  # d id / d t2 = 1 / t2^2
    # ppx = (ph0 / ph3 + 1) W / 2, ppy likewise, ph = P t
    ph = ab(p.ph)
    iw = 1.0 / np.where(p.valid, ph[:, 3], 1.0)
    gnx, gny = gpx * u.W / 2.0, gpy * u.H / 2.0
    gph = np.zeros((n, 4))
    gph[:, 0], gph[:, 1] = gnx * iw, gny * iw
    gph[:, 3] = sgn * (gnx * ph[:, 0] + gny * ph[:, 1]) * iw * iw
    gt = gt + gph @ P
    center = (gt @ MV)[:, :3]
    center[~p.valid], cov[~p.valid] = 0.0, 0.0
    return center, cov


def model_chain(ubo, center, cov, rows):
    """The projection backwards in float64: rows (n, >= 5) = dL/d(ppx, ppy, A, B, C) to dL/d(centre) (n, 3) and dL/d(cov3d)
    (n, 6). With Q = V^-1 = [[A, B], [B, C]] and G = [[dA, dB/2], [dB/2, dC]]: dL/dV = -Q G Q, dL/dSigma = T^T (dL/dV) T,
    dL/dT = 2 (dL/dV) T Sigma, T through J to the view-space position t (J's four entries depend on t0, t1 and 1 / depth),
    (ppx, ppy) through the general P to t, and t = MV (c, 1). Invalid splats get 0. M2: the same chain on absolute values,
    the sum of the absolute values of every product (per output entry). kappa = v00 v11 / det, the conditioning of V^-1."""
    p = project(ubo, center, cov)
    out = ModelChain()
    out.center, out.cov = _chain(p, rows, False)
    out.M2_center, out.M2_cov = _chain(p, rows, True)
    out.valid = p.valid
    out.kappa = np.where(p.valid, p.V[:, 0, 0] * p.V[:, 1, 1] / np.where(p.valid, p.det, 1.0), 0.0)
    return out


def _rotation(rot):
    """R (n, 3, 3) as [n, k, i] (row k, column i), the quaternion polynomial of cor_f64.covariance's Sigma_ij = sum_k s_k^2
    R_ki R_kj with q = (r, x, y, z) as given; Rabs, the same polynomial with every product by its absolute value and every
    difference as a sum; dR[c], the derivative of every entry with respect to q_c, written out entry by entry."""
    q = np.asarray(rot, np.float64)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    o = np.zeros_like(r)

    def mat(rows):
        return np.stack([np.stack(row, -1) for row in rows], -2)

    R = mat([[1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)],
             [2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)],
             [2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)]])
    a = np.abs
    Rabs = mat([[1 + 2 * (y * y + z * z), 2 * (a(x * y) + a(r * z)), 2 * (a(x * z) + a(r * y))],
                [2 * (a(x * y) + a(r * z)), 1 + 2 * (x * x + z * z), 2 * (a(y * z) + a(r * x))],
                [2 * (a(x * z) + a(r * y)), 2 * (a(y * z) + a(r * x)), 1 + 2 * (x * x + y * y)]])
    dR = [mat([[o, 2 * z, -2 * y], [-2 * z, o, 2 * x], [2 * y, -2 * x, o]]),               # d / dr
          mat([[o, 2 * y, 2 * z], [2 * y, -4 * x, 2 * r], [2 * z, -2 * r, -4 * x]]),       # d / dx
          mat([[-4 * y, 2 * x, -2 * r], [2 * x, o, 2 * z], [2 * r, 2 * z, -4 * y]]),       # d / dy
          mat([[-4 * z, 2 * r, 2 * x], [-2 * r, -4 * z, 2 * y], [2 * x, 2 * y, o]])]       # d / dz
    return R, Rabs, dR


def covariance_magnitude(rot, scale):
    """(n, 6) in cov3d order: sum_k s_k^2 Rabs_ki Rabs_kj, the sum of the absolute values of the products that
    cor_f64.covariance's Sigma_ij = sum_k s_k^2 R_ki R_kj sums, R's own polynomial taken apart (Rabs of _rotation)"""
    s = np.asarray(scale, np.float64)
    Rabs = _rotation(rot)[1]
    return cov6(np.einsum("nk,nki,nkj->nij", s * s, Rabs, Rabs))


def scale_chain(r, s, dcov, mcov):
    """dL/d(scale) from dL/d(cov3d) by hand: Sigma_ij = sum_k s_k^2 R_ki R_kj (cor_f64.covariance), so dSigma_ij / ds_k =
    2 s_k R_ki R_kj; a cov3d off-diagonal gradient already counts both places. Second result: the sum of absolute products,
    with R's entries as they are (param_chain's M_scale takes R's own terms apart as well)."""
    R = _rotation(r)[0]
    # R's convention checked against covariance itself
    np.testing.assert_allclose(np.einsum("nk,nki,nkj->nij", s * s, R, R), F.covariance(r, s), rtol=1e-12, atol=1e-18)
    g, m = np.zeros_like(s), np.zeros_like(s)
    for e, (i, j) in enumerate(COV_IJ):
        term = 2 * s * R[:, :, i] * R[:, :, j]  # (n, k)
        g += dcov[:, e, None] * term
        m += mcov[:, e, None] * np.abs(term)
    return g, m


class ParamChain:
    """What param_chain returns: scale (n, 3), rot (n, 4), M_scale, M_rot (the same shapes)"""


def param_chain(rot, scale, dcov, mcov):
    """cov3d backwards to the parameters in float64: dcov (n, 6) = dL/d(cov3d) to dL/d(scale) (n, 3) and dL/d(rot) (n, 4),
    rot = (r, x, y, z) taken as given, not normalised (R is a polynomial in it, and the gradient has a radial part).
    From Sigma_ij = sum_k s_k^2 R_ki R_kj, cov3d slot e = Sigma_ij for (i, j) = COV_IJ[e] (an off-diagonal slot is one
    variable, so dcov[e] is taken once):
        dL/ds_k  = sum_e dcov_e 2 s_k R_ki R_kj
        dL/dR_ka = sum_e dcov_e s_k^2 ([a == i] R_kj + [a == j] R_ki)
        dL/dq_c  = sum_ka dL/dR_ka dR_ka/dq_c
    M_scale, M_rot: the same sums fed mcov (the magnitudes of dcov, e.g. model_chain's M2_cov) with every factor by its
    absolute value and every difference as a sum, R's own polynomial included (Rabs), as _chain(..., absolute=True) forms
    M2 for the projection."""
    s = np.asarray(scale, np.float64)
    dcov, mcov = np.asarray(dcov, np.float64), np.asarray(mcov, np.float64)
    R, Rabs, dR = _rotation(rot)
    out = ParamChain()
    out.scale, out.M_scale = np.zeros_like(s), np.zeros_like(s)
    gR, mR = np.zeros_like(R), np.zeros_like(R)
    s2 = s * s
    for e, (i, j) in enumerate(COV_IJ):
        d, m = dcov[:, e, None], mcov[:, e, None]
        out.scale += d * (2 * s * R[:, :, i] * R[:, :, j])
        out.M_scale += m * (2 * np.abs(s) * Rabs[:, :, i] * Rabs[:, :, j])
        gR[:, :, i] += d * s2 * R[:, :, j]
        gR[:, :, j] += d * s2 * R[:, :, i]
        mR[:, :, i] += m * s2 * Rabs[:, :, j]
        mR[:, :, j] += m * s2 * Rabs[:, :, i]
    out.rot = np.stack([(gR * dR[c]).sum((1, 2)) for c in range(4)], -1)
    out.M_rot = np.stack([(mR * np.abs(dR[c])).sum((1, 2)) for c in range(4)], -1)
    return out
