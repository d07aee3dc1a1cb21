"""The float64 depth backward of tests/cor_f64_depth.py checked on the CPU, on the scene of test_grad_f64.py (the GPU
comparison, tests/test_depth_grad_gpu.py, holds the splat-depth gradient frame and the depth chain to it).

depth_gradients() against central differences of this file's own float64 loss <G, rgba> + <Gdepth, depth> in what a row
differentiates: the opacity, (ppx, ppy, A, B, C) and the centre's view depth of single Gaussians; depth_chain() against
central differences of cor_f64_geom.project(); and the conditions the scene must meet for the GPU comparison to reach
what is new: a clamped hit with a depth weight, a ray that stops early. With Gdepth = 0 the rows are splat_gradients'.
"""
import hashlib

import numpy as np

import cor_f64 as F
import cor_f64_depth as D
import cor_f64_geom as Q
import test_grad_f64 as S

FD_CASE = ("origin", 18, 18, 1)


def upstream_depth(case, seed, with_sh=True):
    """Gdepth (h, w) float32: seeded normal noise, zero on the float32-sensitive pixels like test_grad_f64.upstream's G"""
    _, w, h, _ = case
    G = np.random.default_rng(seed).standard_normal((h, w)).astype(np.float32)
    G[S.sensitive(case, with_sh).near] = 0.0
    return G


def _model():
    c, r, s, o, sh = S.scene()
    return tuple(np.asarray(a, np.float64) for a in (c, r, s, o, sh))


def loss(u, sp, G, Gd):
    """<G, rgba> + <Gd, depth> of the frame of the screen-space splats sp (a cor_f64.Splats, whose fields the caller may
    have moved), and the hash of its hit lists (ray, Gaussian, clamp state, in blend order). Forward only: the blend of
    cor_f64.render with one more channel, z."""
    jit = F.jitter(u.seed, u.S)
    L = 0.0
    digest = hashlib.sha256()
    for (ty, ye, tx, xe), cand, xs, ys in F._tiles(u, sp, 0, u.H, 16):
        m = len(xs)
        tile_near = np.zeros(m, bool)
        iy, ix = ys.astype(np.int64), xs.astype(np.int64)
        for s, (jx, jy) in enumerate(jit):
            if not len(cand):
                continue
            px, py = xs + jx, ys + jy
            o, d = F.rays(u, px, py)
            h = F._hits(sp, cand, px, py, o, d, tile_near, 1e-3, 1e-5, 1e-6)
            C, T, _ = F._walk(h, m, tile_near, 1e-3)
            b = h.blended
            r, g = h.ri[b], h.gi[b]
            digest.update(((iy[r] * u.W + ix[r]) * u.S + s).tobytes() + g.tobytes() + (h.oe[b] < 0.99).tobytes())
            Dz = np.bincount(r, weights=sp.depth[g] * h.alpha[b] * h.T[b], minlength=m)
            L += ((G[iy, ix, :3] * C).sum() + (G[iy, ix, 3] * (1.0 - T)).sum() + (Gd[iy, ix] * Dz).sum()) / u.S
    return L, digest.hexdigest()


def test_rows_match_central_differences():
    """For the eight Gaussians with the largest M (slots 0..6 summed), 18x18 at 1 spp, G and Gdepth zero on the
    float32-sensitive pixels: each of the seven variables of a row moved alone. A step starts at 1e-5 (times the conic's
    size for A, B, C) and is halved until the hit lists, their order and the clamp states at +h and -h are the base
    frame's, which is asserted. Bound: 1e-6 M, as test_geom_grad_f64 holds splat_gradients."""
    c, r, s, o, sh = _model()
    ubo = S.camera(*FD_CASE)
    u = F.Ubo(ubo)
    G = S.upstream(FD_CASE, 4, 61).astype(np.float64)
    Gd = upstream_depth(FD_CASE, 62).astype(np.float64)
    dg = D.depth_gradients(ubo, c, r, s, o, sh, G_rgba=G, G_depth=Gd)
    sp = F.Splats(u, c, r, s, o, sh)
    base, base_digest = loss(u, sp, G, Gd)
    assert base_digest == dg.digest
    np.testing.assert_allclose((Gd * dg.depth).sum() + (G * F.render(ubo, c, r, s, o, sh)[0]).sum(), base, rtol=1e-12)
    picked = np.argsort(-dg.M[:, :7].sum(1))[:8]
    assert (dg.M[picked, :7] > 0).all()
    fields = ["ppx", "ppy", "ca", "cb", "cc", "opacity", "depth"]  # slots 0..6
    worst = 0.0
    for g in picked:
        conic = 0.5 * (sp.ca[g] + sp.cc[g])
        for k, name in enumerate(fields):
            h = 1e-5 * (conic if name in ("ca", "cb", "cc") else 1.0)
            arr = getattr(sp, name)
            keep = arr[g]
            for _ in range(12):
                side = []
                for sign in (-1.0, 1.0):
                    arr[g] = keep + sign * h
                    L, dig = loss(u, sp, G, Gd)
                    if dig != base_digest:
                        break
                    side.append(L)
                arr[g] = keep
                if len(side) == 2:
                    break
                h /= 2
            assert len(side) == 2, (int(g), name, "no step keeps the hit sets")
            fd = (side[1] - side[0]) / (2 * h)
            err = abs(fd - dg.rows[g, k]) / dg.M[g, k]
            worst = max(worst, err)
            assert err <= 1e-6, (int(g), name, h, fd, dg.rows[g, k], dg.M[g, k])
    print(f"depth rows against central differences: worst error / M = {worst:.3g}")
    assert (np.abs(dg.rows) <= dg.M * (1 + 1e-12)).all() and not dg.rows[:, 7].any() and not dg.M[:, 7].any()


def test_depth_chain_matches_central_differences():
    """L = sum_g <f_g, (ppx, ppy, A, B, C, -, depth)_g> with random f, as test_geom_grad_f64 holds model_chain: steps 1e-5
    in a centre coordinate and 1e-5 of the Gaussian's mean variance in a cov3d entry, bound 1e-6 M2."""
    c, r, s, o, _ = _model()
    ubo = S.camera("moved", 48, 32, 1)
    cov = Q.cov6(F.covariance(r, s))
    f = np.zeros((S.N, 8))
    f[:, [0, 1, 2, 3, 4, 6]] = np.random.default_rng(33).uniform(-1.0, 1.0, (S.N, 6))
    got = D.depth_chain(ubo, c, cov, f)
    plain = Q.model_chain(ubo, c, cov, f)
    v = got.valid
    assert v.sum() > 100
    assert np.array_equal(got.cov, plain.cov) and np.array_equal(got.M2_cov, plain.M2_cov)  # nothing flows to cov3d
    assert (got.center[v] != plain.center[v]).any()

    def L(cc, vv):
        p = Q.project(ubo, cc, vv)
        assert np.array_equal(p.valid, v)
        return np.stack([p.ppx, p.ppy, p.A, p.B, p.C, p.depth], -1) * f[:, [0, 1, 2, 3, 4, 6]]

    worst = 0.0
    for k in range(3):
        h = 1e-5
        d = np.zeros_like(c)
        d[:, k] = h
        fd = (L(c + d, cov) - L(c - d, cov)).sum(1) / (2 * h)
        worst = max(worst, (np.abs(fd - got.center[:, k])[v] / got.M2_center[:, k][v]).max())
    hs = 1e-5 * cov[:, [0, 3, 5]].mean(1)
    for k in range(6):
        d = np.zeros_like(cov)
        d[:, k] = hs
        fd = (L(c, cov + d) - L(c, cov - d)).sum(1) / (2 * hs)
        worst = max(worst, (np.abs(fd - got.cov[:, k])[v] / got.M2_cov[:, k][v]).max())
    print(f"depth_chain against central differences: worst error / M2 = {worst:.3g}")
    assert worst <= 1e-6
    assert (np.abs(got.center) <= got.M2_center * (1 + 1e-12)).all()
    assert not got.center[~v].any() and not got.cov[~v].any()


def test_scene_reaches_the_depth_terms():
    """On the GPU comparison's inputs: a clamped hit carries slot-6 weight, a ray stops early, and some Gaussian takes more
    than 40 TOL of its blend weight through clamped hits, so a slot 6 without them misses the GPU bound forty times over
    (none of this scene's Gaussians is only ever clamped under any camera of CASES: a splat clamped near its centre is open
    at its rim); with Gdepth = 0 slots 0..5 are splat_gradients' exactly and slot 6 is 0; with
    G = 0 and Gdepth = 1 slot 6 is the summed blend weight, and the weights times z sum to the depth image."""
    c, r, s, o, sh = _model()
    case = S.CASES[0]
    ubo = S.camera(*case)
    G = S.upstream(case, 4, 63)
    Gd = upstream_depth(case, 64)
    dg = D.depth_gradients(ubo, c, r, s, o, sh, G_rgba=G, G_depth=Gd)
    assert dg.counts["clamped_depth_hits"] > 0 and dg.counts["stopped_rays"] > 0
    assert (dg.weight_clamped > 40 * S.TOL * dg.weight).any() and (dg.weight_clamped <= dg.weight).all()
    assert np.array_equal(dg.near, S.sensitive(case).near)
    zero = D.depth_gradients(ubo, c, r, s, o, sh, G_rgba=G, G_depth=np.zeros_like(Gd))
    sg = Q.splat_gradients(ubo, c, r, s, o, sh, G_rgba=G)
    assert zero.digest == sg.digest
    assert np.array_equal(zero.rows[:, :6], sg.rows[:, :6]) and np.array_equal(zero.M[:, :6], sg.M[:, :6])
    assert not zero.rows[:, 6:].any()
    ones = D.depth_gradients(ubo, c, r, s, o, sh, G_rgba=np.zeros_like(G), G_depth=np.ones_like(Gd))
    np.testing.assert_allclose(ones.rows[:, 6], ones.weight, rtol=1e-12, atol=0)
    sp = F.Splats(F.Ubo(ubo), c, r, s, o, sh)
    np.testing.assert_allclose((ones.weight * sp.depth).sum(), ones.depth.sum(), rtol=1e-12)
    assert np.array_equal(ones.depth, dg.depth) and (dg.depth_M >= np.abs(dg.depth)).all() and dg.depth.max() > 0
