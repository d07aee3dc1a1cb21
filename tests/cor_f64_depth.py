"""The float64 expected depth of a COR frame and its backward -- test infrastructure beside tests/cor_f64_geom.py.

The depth image is D = sum_i z_i w_i per sample ray, over the hits cor_f64's blend takes and with its weights, averaged over
a pixel's samples as the colour is; z_i is the view depth of Gaussian i's centre (cor_f64.Splats.depth, the key of the hit
order). depth_gradients is the backward of L = <G, rgba> + <Gdepth, depth> to the eight-slot rows of
gsrt_render_splat_depth_grad (include/gsrt.h), built on cor_f64's hit lists (_tiles, _hits, _walk: imported, not copied) as
cor_f64_geom.splat_gradients is; depth_chain takes such rows through the projection, slot 6 included.

Everything is numpy float64. Nothing here shares a value or an operation order with the HIP kernels.
"""
import hashlib

import numpy as np

import cor_f64 as F
import cor_f64_geom as Q


class DepthGradients:
    """What depth_gradients returns: rows (n, 8), M (n, 8); depth (rows, W), the float64 depth image, and depth_M, its
    per-pixel sum of |z_i| w_i (both over ns); weight (n,), every Gaussian's blend weight summed over the frame (over ns),
    and weight_clamped, the part of it from hits whose alpha the clamp replaced;
    near (rows, W) bool; digest (cor_f64.gradients' hash of the hit lists); gauss_clamped, gauss_open (n,) bool: the
    Gaussian has a clamped / an open blended hit; counts: dict of stopped_rays, clamped_depth_hits (clamped hits whose
    slot-6 term is non-zero)"""


def depth_gradients(ubo, center, rot, scale, opacity, sh=None, *, G_rgba, G_depth, rows=None, tile=16, alpha_rel=1e-3,
                    trans_rel=1e-3, slab_rel=1e-5, depth_rel=1e-6, col_rel=1e-4):
    """The rows of gsrt_render_splat_depth_grad in float64. Depth is one more blended channel whose colour is z_i:
        d D / d alpha_i = T_i z_i - SD_i / (1 - alpha_i),  SD_i = sum_{j>i} z_j w_j (summed from the ray's last hit backwards)
        d_i = (cor_f64_geom.splat_gradients' d_i) + Gd (T_i z_i - SD_i / (1 - alpha_i)),  Gd = Gdepth[p] / ns
    slots 0..5 are splat_gradients' formulas with this d_i, on the hits with o e_i < 0.99; and z_i is a variable of its own,
        rows[g, 6] += w_i Gd      on every blended hit, clamped or not (d D / d z_i = w_i),
    slot 7 stays 0. M sums the absolute value of every product: mag_i gains |Gd| (T_i |z_i| + SD|.|_i / (1 - alpha_i)) with
    SD|.| the same backward sum of |z_j| w_j, slots 0..5 follow splat_gradients from it, and slot 6 gets |w_i Gd|."""
    u = F.Ubo(ubo)
    sp = F.Splats(u, center, rot, scale, opacity, sh)
    n = sp.n
    r0, r1 = rows if rows else (0, u.H)
    near = np.zeros((u.H, u.W), bool)
    jit = F.jitter(u.seed, u.S)
    Gr = np.asarray(G_rgba, np.float64).reshape(u.H, u.W, 4) / u.S
    Gz = np.asarray(G_depth, np.float64).reshape(u.H, u.W) / u.S
    out = DepthGradients()
    out.rows, out.M = np.zeros((n, 8)), np.zeros((n, 8))
    out.weight, out.weight_clamped = np.zeros(n), np.zeros(n)
    depth, depth_M = np.zeros((u.H, u.W)), np.zeros((u.H, u.W))
    g_clamped, g_open = np.zeros(n, bool), np.zeros(n, bool)
    cnt = dict(stopped_rays=0, clamped_depth_hits=0)
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
            _, T_end, stopped = F._walk(h, m, tile_near, trans_rel)
            F._clamps_near(sp, h, tile_near, alpha_rel, col_rel)
            b = h.blended
            r, g, a, Ti, col, e = h.ri[b], h.gi[b], h.alpha[b], h.T[b], h.col[b], h.e[b]
            is_open = h.oe[b] < 0.99
            digest.update(((iy[r] * u.W + ix[r]) * u.S + s).tobytes() + g.tobytes() + is_open.tobytes())
            cnt["stopped_rays"] += int(stopped.sum())
            g_clamped[g[~is_open]] = True
            g_open[g[is_open]] = True
            w = a * Ti
            z = sp.depth[g]
            starts = np.searchsorted(r, np.arange(m))
            counts = np.bincount(r, minlength=m)
            # the colour, the depth and the absolute depth behind each hit, from the ray's last hit backwards
            S, SD, SDa = np.zeros((len(r), 3)), np.zeros(len(r)), np.zeros(len(r))
            behind, behind_z, behind_za = np.zeros((m, 3)), np.zeros(m), np.zeros(m)
            for k in range(int(counts.max()) - 1 if len(r) else -1, -1, -1):
                rr = np.nonzero(counts > k)[0]
                p = starts[rr] + k
                S[p], SD[p], SDa[p] = behind[rr], behind_z[rr], behind_za[rr]
                behind[rr] += col[p] * w[p, None]
                behind_z[rr] += z[p] * w[p]
                behind_za[rr] += np.abs(z[p]) * w[p]
            np.add.at(depth, (iy, ix), behind_z / u.S)  # after the loop: the whole ray's sum
            np.add.at(depth_M, (iy, ix), behind_za / u.S)
            Gs, Gd = Gr[iy[r], ix[r]], Gz[iy[r], ix[r]]
            rinv = 1.0 / (1.0 - a)
            front, back = Ti[:, None] * col, S * rinv[:, None]
            tail = T_end[r] * rinv
            dLda = (Gs[:, :3] * (front - back)).sum(1) + Gs[:, 3] * tail + Gd * (Ti * z - SD * rinv)
            mag = ((np.abs(Gs[:, :3]) * (front + back)).sum(1) + np.abs(Gs[:, 3]) * tail +
                   np.abs(Gd) * (Ti * np.abs(z) + SDa * rinv))
            dx, dy = px[r] - sp.ppx[g], py[r] - sp.ppy[g]
            A, B, C = sp.ca[g], sp.cb[g], sp.cc[g]
            q, qm = -a * dLda, a * mag
            zero = 0 * q
            terms = np.stack([q * -(A * dx + B * dy), q * -(B * dx + C * dy), q * 0.5 * dx * dx, q * dx * dy,
                              q * 0.5 * dy * dy, dLda * e, zero, zero], -1)
            mags = np.stack([qm * (np.abs(A * dx) + np.abs(B * dy)), qm * (np.abs(B * dx) + np.abs(C * dy)),
                             qm * 0.5 * dx * dx, qm * np.abs(dx * dy), qm * 0.5 * dy * dy, mag * e, zero, zero], -1)
            F._scatter(out.rows, g[is_open], terms[is_open])
            F._scatter(out.M, g[is_open], mags[is_open])
            tz = w * Gd  # every blended hit
            F._scatter(out.rows[:, 6], g, tz)
            F._scatter(out.M[:, 6], g, np.abs(tz))
            F._scatter(out.weight, g, w / u.S)
            F._scatter(out.weight_clamped, g[~is_open], (w / u.S)[~is_open])
            cnt["clamped_depth_hits"] += int(((~is_open) & (tz != 0)).sum())
        near[ty:ye, tx:xe] = tile_near.reshape(ye - ty, xe - tx)
    out.near, out.digest, out.counts = near[r0:r1], digest.hexdigest(), cnt
    out.depth, out.depth_M = depth[r0:r1], depth_M[r0:r1]
    out.gauss_clamped, out.gauss_open = g_clamped, g_open
    return out


def depth_chain(ubo, center, cov, rows):
    """cor_f64_geom.model_chain with the depth slot: depth = -t_2, t = MV (c, 1), so dL/dt_2 gains -rows[:, 6] and the
    centre -rows[:, 6] (row 2 of MV's 3x3); cov3d gains nothing. M2_center gains |rows[:, 6]| |MV row 2|. Invalid splats
    get 0."""
    rows = np.asarray(rows, np.float64)
    out = Q.model_chain(ubo, center, cov, rows)
    u = F.Ubo(ubo)
    v = out.valid[:, None]
    out.center = out.center + np.where(v, -rows[:, 6, None] * u.MV[2, :3][None, :], 0.0)
    out.M2_center = out.M2_center + np.where(v, np.abs(rows[:, 6, None]) * np.abs(u.MV[2, :3])[None, :], 0.0)
    return out
