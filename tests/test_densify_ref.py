"""The numpy reference of adaptive density control (tests/densify_ref.py) and the inputs the GPU comparison uses
(tests/test_densify_gpu.py), checked on the CPU: every decision occurs on the test model, origin and the row order are
consistent with the counts, the statistic treats zeros, -0 and NaN as the header says, and a split's samples have the
scene's own covariance (R, not its transpose)."""
import numpy as np
import torch

import densify_ref as D
import test_grad_f64 as S
from gsrt.autograd import model_covariance


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_every_decision_occurs_on_the_test_model():
    """On the 300-Gaussian model with the GPU tests' synthetic stats and thresholds: keep, clone, split, prune by opacity
    and prune by scale each at least 10 times."""
    (c, r, s, o, sh, feat), stats, noise, P, ref = D.case(S.N)
    rows, split, clone, by_opacity, by_scale = D.decide(s, o, stats, P)
    kinds = {"keep": int((rows == 1).sum()), "clone": int(clone.sum()), "split": int(split.sum()),
             "prune by opacity": int(by_opacity.sum()), "prune by scale": int(by_scale.sum())}
    print(kinds)
    assert all(v >= 10 for v in kinds.values()), kinds
    assert np.isnan(o[7]) and by_opacity[7] and rows[7] == 0  # a NaN opacity is pruned
    assert ref.n_out == int(rows.sum()) == kinds["keep"] + 2 * (kinds["clone"] + kinds["split"])


def test_origin_and_order():
    (c, r, s, o, sh, feat), stats, noise, P, ref = D.case(1025)
    rows, split, clone, _, _ = D.decide(s, o, stats, P)
    own = ref.origin[ref.origin >= 0]
    assert np.array_equal(own, np.nonzero(rows > 0)[0][~split[rows > 0]])  # kept and cloned Gaussians, in input order
    fresh = -1 - ref.origin[ref.origin < 0]
    assert np.array_equal(np.bincount(fresh, minlength=1025), np.where(split, 2, np.where(clone, 1, 0)))
    parent = np.where(ref.origin >= 0, ref.origin, -1 - ref.origin)
    assert (np.diff(parent) >= 0).all() and np.array_equal(np.bincount(parent, minlength=1025), rows)
    # copies keep every bit; a split moves the centre and shrinks the scales only
    copy = np.isin(parent, np.nonzero(~split)[0])
    for got, src in ((ref.center, c), (ref.scale, s)):
        assert np.array_equal(u32(got[copy]), u32(src[parent[copy]]))
        assert (u32(got[~copy]) != u32(src[parent[~copy]])).any(axis=1).all()
    for got, src in ((ref.rot, r), (ref.opacity, o), (ref.sh, sh), (ref.features, feat)):
        assert np.array_equal(u32(got), u32(src[parent]))
    assert np.array_equal(u32(ref.scale[~copy]), u32(s[parent[~copy]] / np.float32(1.6)))


def test_identity_all_split_all_prune():
    (c, r, s, o, sh, feat), stats, noise, _, _ = D.case(S.N)
    same = D.densify(c, r, s, o, sh, feat, stats, noise, D.params(np.inf, 0.0, 0.0, 0.0))
    assert same.n_out == S.N - 1 and np.array_equal(same.origin, np.delete(np.arange(S.N), 7))  # the NaN opacity goes
    o1 = np.where(np.isnan(o), np.float32(0.5), o)
    same = D.densify(c, r, s, o1, sh, feat, stats, noise, D.params(np.inf, 0.0, 0.0, 0.0))
    assert same.n_out == S.N and np.array_equal(u32(same.center), u32(c)) and np.array_equal(u32(same.sh), u32(sh))
    ones = np.ones((S.N, 2), np.float32)
    assert D.densify(c, r, s, o1, sh, feat, ones, noise, D.params(0.0, 0.0, 0.0, 0.0)).n_out == 2 * S.N
    assert D.densify(c, r, s, o1, sh, feat, ones, noise, D.params(0.0, 0.0, 2.0, 0.0)).n_out == 0


def test_stats_add_zero_minus_zero_nan():
    rows = np.zeros((6, 8), np.float32)
    rows[1, :6] = -0.0                      # not seen
    rows[2, 3] = np.nan                     # seen, norm 0
    rows[3, :2] = (3.0, -4.0)               # seen, norm of (3 * 8, -4 * 4)
    rows[4, 6:] = 5.0                       # slots 6 and 7 do not count
    rows[5, 0] = np.nan                     # seen, a NaN norm
    start = np.full((6, 2), 7.0, np.float32)
    start[0] = (-0.0, np.nan)
    got = D.stats_add(rows, start, 16, 8)
    assert np.array_equal(u32(got[[0, 1, 4]]), u32(start[[0, 1, 4]]))
    assert got[2].tolist() == [7.0, 8.0] and got[3].tolist() == [7.0 + np.float32(np.sqrt(np.float32(832.0))), 8.0]
    assert np.isnan(got[5, 0]) and got[5, 1] == 8.0
    again = D.stats_add(rows, got, 16, 8)
    assert again[3, 1] == 9.0 and again[3, 0] == got[3, 0] + np.float32(np.sqrt(np.float32(832.0)))


def test_split_samples_have_the_scene_covariance():
    """One anisotropic, rotated Gaussian split 100 000 times with normal noise: 200 000 draws of x = centre' - centre.
    Their second moment (the mean is known to be 0) against Sigma of gsrt.autograd.model_covariance. For a normal x the
    estimate of Sigma_ij from N draws has variance (Sigma_ii Sigma_jj + Sigma_ij^2) / N; the bound is 5 such standard
    errors per entry. With R transposed the off-diagonal entries are off by their own size, hundreds of standard errors."""
    n = 100_000
    N = 2 * n
    q = np.array([0.8, 0.3, -0.4, 0.33], np.float64)
    rot = np.tile((q / np.linalg.norm(q)).astype(np.float32), (n, 1))
    scale = np.tile(np.array([0.9, 0.25, 0.05], np.float32), (n, 1))
    center = np.zeros((n, 3), np.float32)
    noise = np.random.default_rng(73).standard_normal((n, 2, 3)).astype(np.float32)
    ones = np.ones((n, 2), np.float32)
    ref = D.densify(center, rot, scale, np.ones(n, np.float32), None, None, ones, noise, D.params(0.5, 0.1, 0.0, 0.0, 1.6))
    assert ref.n_out == N and (ref.origin < 0).all()
    x = ref.center.astype(np.float64)
    got = x.T @ x / N
    cov = model_covariance(torch.from_numpy(rot[:1]).double(), torch.from_numpy(scale[:1]).double())[0].numpy()
    Sigma = np.array([[cov[0], cov[1], cov[2]], [cov[1], cov[3], cov[4]], [cov[2], cov[4], cov[5]]])
    se = np.sqrt((np.outer(np.diag(Sigma), np.diag(Sigma)) + Sigma ** 2) / N)
    print("worst |sample - Sigma| / standard error:", float((np.abs(got - Sigma) / se).max()))
    assert (np.abs(got - Sigma) <= 5.0 * se).all()
    # the power of the check: the transposed convention misses the bound by far
    R = np.array([[float(e[0]) for e in row] for row in D.rotation(rot[:1])])
    wrong = (np.diag(scale[0].astype(np.float64)) @ R.T).T @ (np.diag(scale[0].astype(np.float64)) @ R.T)
    assert (np.abs(wrong - Sigma) > 50.0 * se).any()
