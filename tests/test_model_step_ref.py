"""tests/model_step_ref.py checked on the CPU: adam_ref against torch.optim.Adam in float64, chain_f64 against torch
autograd of normalise -> exp -> model_covariance in float64, gsrt.adam_scalars against Python doubles rounded once, and the
inputs of case(300) for what they claim.

adam_ref's bound. With d = 2^-24, the float32 scalars a1, a2, c2, ss each rounded once from the doubles torch uses, beta1,
beta2, eps the same float32 values on both sides, and first-order error terms:
    m' = beta1 m + a1 g:    two products, a1's rounding, one sum: |dm'| <= 3 d Mm,  Mm = |beta1 m| + |a1 g|
    v' = beta2 v + (a2 g) g: three products, a2's rounding, one sum: |dv'| <= 4 d v'  (every term is >= 0)
    den = sqrt(v') / c2 + eps: the root halves v's 4 d and adds 1, c2's rounding 1, the division 1, the sum 1: <= 6 d den
    num = ss m': ss's rounding 1, the product 1, m's 3 d Mm: |dnum| <= 5 d ss Mm
    u = num / den: (5 + 6 + 1) d ss Mm / den;  p' = p - u: one more rounding of p', |p'| <= |p| + |u|
    |dp'| <= d (|p| + 13 ss Mm / den)
13 rounded operations (the nine of the formulas' own products, sums, root and quotients on the path to p', and the four
scalars' roundings) reach the step and one the parameter. The second-order terms are below 13^2 d^2, covered by a factor
1.001.
"""
import math

import numpy as np
import pytest

import gsrt
import model_step_ref as R

EPS = R.EPS


@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_ref_against_torch_float64(t):
    import torch

    rng = np.random.default_rng(t)
    n = 4096
    p = rng.normal(0, 1, n).astype(np.float32)
    m = rng.normal(0, 0.05, n).astype(np.float32)
    v = rng.uniform(0, 0.01, n).astype(np.float32)
    g = (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 0, n)).astype(np.float32)
    if t == 1:
        m[:], v[:] = 0.0, 0.0  # a first step starts from zero moments
    lr = 1e-3
    adam = gsrt.adam_params(lr_center=lr, step=t)
    a1, a2, c2, ss = gsrt.adam_scalars(adam)[:4]
    p2, m2, v2 = R.adam_ref(p, m, v, g, adam.beta1, adam.beta2, adam.eps, a1, a2, c2, ss)

    b1, b2, eps = float(adam.beta1), float(adam.beta2), float(adam.eps)
    tp = torch.tensor(p.astype(np.float64), requires_grad=True)
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    opt.state[tp] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.tensor(m.astype(np.float64)),
                         exp_avg_sq=torch.tensor(v.astype(np.float64)))
    tp.grad = torch.tensor(g.astype(np.float64))
    opt.step()
    want_p = tp.detach().numpy()
    want_m, want_v = opt.state[tp]["exp_avg"].numpy(), opt.state[tp]["exp_avg_sq"].numpy()

    p64, m64, g64 = (a.astype(np.float64) for a in (p, m, g))
    Mm = np.abs(b1 * m64) + np.abs((1 - b1) * g64)
    den = np.sqrt(want_v) / math.sqrt(1 - b2 ** t) + eps
    step_size = lr / (1 - b1 ** t)
    slack = 1.001
    assert (np.abs(m2 - want_m) <= slack * 3 * EPS * Mm).all()
    assert (np.abs(v2 - want_v) <= slack * 4 * EPS * want_v).all()
    bound = slack * EPS * (np.abs(p64) + 13 * step_size * Mm / den)
    err = np.abs(p2.astype(np.float64) - want_p)
    print(f"t = {t}: worst error / bound = {(err / bound).max():.3g}")
    assert (err <= bound).all()
    assert (p2 != p).mean() > 0.5  # the step moved the parameters: the comparison is not of two copies


def test_adam_ref_is_float32_op_by_op():
    """one word by hand, every intermediate rounded with np.float32"""
    f = np.float32
    p, m, v, g = f(0.3), f(0.01), f(2e-4), f(-0.7)
    b1, b2, eps, a1, a2, c2, ss = f(0.9), f(0.999), f(1e-15), f(0.1), f(0.001), f(0.5), f(0.01)
    m2 = f(f(b1 * m) + f(a1 * g))
    v2 = f(f(b2 * v) + f(f(a2 * g) * g))
    p2 = f(p - f(f(ss * m2) / f(f(np.sqrt(v2) / c2) + eps)))
    got = R.adam_ref(np.array([p]), np.array([m]), np.array([v]), np.array([g]), b1, b2, eps, a1, a2, c2, ss)
    assert [a[0].view(np.uint32) for a in got] == [x.view(np.uint32) for x in (p2, m2, v2)]


def test_chain_f64_against_torch_autograd():
    import torch

    from gsrt.autograd import model_covariance

    k = R.case(300)
    rot, ls, logit = (a.astype(np.float64) for a in k.raw[1:4])
    rot[k.zero_quat] = [0.3, -0.2, 0.9, 0.4]  # autograd of the normalisation has no value at 0: checked apart below
    rng = np.random.default_rng(3)
    dcov, dop = rng.uniform(-1, 1, (300, 6)), rng.uniform(-1, 1, 300)
    t_r, t_s, t_o = (torch.tensor(a, requires_grad=True) for a in (rot, ls, logit))
    q = t_r / t_r.norm(dim=1, keepdim=True)
    cov = model_covariance(q, torch.exp(t_s))
    loss = (cov * torch.tensor(dcov)).sum() + (torch.sigmoid(t_o) * torch.tensor(dop)).sum()
    g_r, g_s, g_o = torch.autograd.grad(loss, (t_r, t_s, t_o))
    c = R.chain_f64(rot, ls, logit, dcov, dop)
    for got, ref, M in ((g_r, c.rot, c.M_rot), (g_s, c.scale, c.M_scale), (g_o, c.opacity, c.M_opacity)):
        np.testing.assert_allclose(got.numpy(), ref, rtol=1e-12, atol=0)
        assert (M >= np.abs(ref) * (1 - 1e-12)).all()  # a magnitude sum is at least its entry
    z = R.chain_f64(np.zeros((1, 4)), ls[:1], logit[:1], dcov[:1], dop[:1])
    assert not z.rot.any() and not z.M_rot.any() and z.scale.any()


def test_adam_scalars_against_python_doubles():
    for t, b1, b2 in ((1, 0.9, 0.999), (2, 0.9, 0.999), (1000, 0.9, 0.999), (7, 0.0, 0.5), (4000000000, 0.5, 0.25)):
        adam = gsrt.adam_params(1.6e-4, 1e-3, 5e-3, 5e-2, 2.5e-3, 1.25e-4, 0.0, b1, b2, 1e-15, t)
        b1f, b2f = float(np.float32(b1)), float(np.float32(b2))
        lrs = [float(getattr(adam, "lr_" + g)) for g in R.GROUPS]
        want = [1 - b1f, 1 - b2f, math.sqrt(1 - b2f ** t)] + [lr / (1 - b1f ** t) for lr in lrs]
        got = gsrt.adam_scalars(adam)
        assert got.dtype == np.float32 and got.shape == (gsrt.ADAM_SCALARS,)
        assert got.view(np.uint32).tolist() == np.array(want, np.float64).astype(np.float32).view(np.uint32).tolist(), t


def test_case_inputs():
    k = R.case(300)
    splat = k.grads[2]
    assert k.special and k.n == 300
    assert (splat[k.neg0_row, :6] == 0).all() and np.signbit(splat[k.neg0_row, :6]).all() and not k.seen[k.neg0_row]
    assert np.isnan(splat[k.nan_row, 0]) and not splat[k.nan_row, 1:6].any() and k.seen[k.nan_row]
    assert not k.raw[1][k.zero_quat].any() and (np.abs(k.raw[1]).sum(1) > 0).sum() == 299
    assert k.seen.sum() >= 50 and (~k.seen).sum() >= 50
    assert splat[~k.seen, 6].any()  # slot 6 is set on unseen rows: only slots 0..5 decide
    adam = k.adam(gsrt)
    assert [g for g in R.GROUPS if getattr(adam, "lr_" + g) == 0.0] == ["scale"]
    norms = np.sqrt((k.raw[1].astype(np.float64) ** 2).sum(1))
    keep = np.arange(300) != k.zero_quat
    assert norms[keep].min() >= 0.49 and norms[keep].max() <= 2.01 and np.ptp(norms[keep]) > 1.0
    assert all((a >= 0).all() for a in k.v if a is not None) and np.isfinite(k.raw[3]).all()
    assert R.case(300) is k and R.case(1025).n == 1025 and R.case(1025).raw[0][300:].any()
    c5 = R.case(65, with_sh=False, channels=5)
    assert c5.raw[4] is None and c5.raw[5].shape == (65, 5) and c5.grads[4].shape == (65, 5)
