"""The optimiser step on the device (gsrt.model_step, model_activate, model_deactivate, model_opacity_reset) against
tests/model_step_ref.py.

Sizes: n in {0, 1, 63, 64, 65, 300, 1025}: a partly filled wave and a full one, a second wave, a second 256-lane workgroup,
a workgroup with one Gaussian in it; the flat row kernel has SH rows straddling workgroups from n = 22 on (256 float4 lanes
hold 21 1/3 rows).

1. Adam is bit-exact: raw', m', v' equal adam_ref fed the returned grad_raw (geometry) and the tables (sh, features), NaNs
   as NaNs; unseen Gaussians (sparse) and the lr = 0 group keep every bit.
2. The scene arrays are the scene build's, bit for bit, and act.rot is the numpy normalisation.
3. Activations and chain against float64, |got - ref| <= N 2^-24 M with N the rounded operations counted in
   gsrt_model_step.hip (model_step_ref.N_ACT, N_CHAIN) and M the magnitude sums of chain_f64. Worst error / bound is printed
   and appended to COR_F64_REPORT; measured: DESIGN.md section 5.
4. Opacity reset bit-exact against numpy; deactivate against float64 and the round trip through activate:
     log scale: logf's E_LOG |log s|; logit = logf(o / (1 - o)): 1 - o (1), the quotient (1) move the logarithm's argument
     by 2 EPS relatively, i.e. the result by 2 EPS, + E_LOG |logit|.
     round trip: s carries E_EXP EPS relatively: E_EXP EPS on log s; o carries (E_EXP + 2) EPS o, d logit / d o =
     1 / (o (1 - o)): (E_EXP + 2) EPS / (1 - o) on the logit; each plus the direct bound above.
5. End to end on 300 Gaussians, 48x32, 4 spp: the bit-exact check on real gradient tables, then 10 steps of the torch-free
   loop lower the loss, and so do 10 steps of render_model + torch.optim.Adam at the same rates.
6. Refusals that need a context.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import gsrt
import model_step_ref as R
import test_grad_f64 as S
import test_grad_f64_gpu as TG
from test_features_gpu import u32

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 300, 1025]
EPS = R.EPS


def same_bits(got, want):
    """bit for bit, a NaN for a NaN"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape
    both_nan = np.isnan(got) & np.isnan(want)
    return bool(((u32(got) == u32(want)) | both_nan).all())


def run_step(ctx, k, sparse, step=1, want_grad_raw=True):
    raw, m, v = k.copies()
    adam = k.adam(gsrt, step=step, sparse=sparse)
    out = gsrt.model_step(ctx, raw, m, v, k.grads, adam, want_grad_raw=want_grad_raw)
    return raw, m, v, adam, out


def expected(k, adam, grad_raw, sparse):
    return R.step_ref(k.raw, k.m, k.v, grad_raw, k.grads[3], k.grads[4], adam, gsrt.adam_scalars(adam),
                      k.seen if sparse else None)


def hold_step(k, got, want, adam, sparse):
    names = ("center", "rot", "scale", "opacity", "sh", "features")
    for which, (g3, w3, before) in zip(("raw", "m", "v"), zip(got, want, (k.raw, k.m, k.v))):
        for name, g, w, b in zip(names, g3, w3, before):
            if g is None:
                assert w is None
                continue
            assert same_bits(g, w), (which, name, k.n, sparse)
            if sparse and k.n:
                assert u32(g)[~k.seen].tobytes() == u32(b)[~k.seen].tobytes(), (which, name)  # unseen: every bit kept
    assert u32(got[0][2]).tobytes() == u32(k.raw[2]).tobytes()  # the lr = 0 group (log scale) kept every bit,
    assert u32(got[1][2]).tobytes() == u32(k.m[2]).tobytes() and u32(got[2][2]).tobytes() == u32(k.v[2]).tobytes()
    assert adam.lr_scale == 0.0


MODELS = pytest.mark.parametrize("with_sh,channels", [(True, 0), (False, 0), (False, 5), (True, 8)],
                                 ids=["sh", "plain", "features5", "sh-features8"])


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@MODELS
@pytest.mark.parametrize("n", SIZES)
def test_adam_is_bit_exact(ctx, n, with_sh, channels, sparse):
    k = R.case(n, with_sh=with_sh, channels=channels)
    raw, m, v, adam, out = run_step(ctx, k, sparse)
    graw = out["grad_raw"]
    assert graw.shape == (n, 11) and u32(graw[:, :3]).tobytes() == u32(k.grads[0]).tobytes()  # d centre is grads.center
    hold_step(k, (raw, m, v), expected(k, adam, graw, sparse), adam, sparse)
    if n >= 8:
        moved = u32(raw[0]) != u32(k.raw[0])
        assert moved[k.seen].any() and (moved[~k.seen].any() != sparse)  # the step moved what it should
        assert np.isfinite(raw[3][k.nan_row]) and (sparse is False or not moved[k.neg0_row].any())
        assert moved[k.nan_row].any()  # a NaN in slot 0 is seen


def test_step_numbers_beyond_the_first(ctx):
    k = R.case(300)
    for t in (2, 1000):
        raw, m, v, adam, out = run_step(ctx, k, True, step=t)
        hold_step(k, (raw, m, v), expected(k, adam, out["grad_raw"], True), adam, True)


def test_device_form_through_torch(ctx):
    """n = 1025 through gsrt.autograd.model_step (device pointers, the async form): the host form's bits"""
    import torch

    from gsrt.autograd import model_step

    k = R.case(1025, with_sh=True, channels=8)
    raw, m, v, adam, out = run_step(ctx, k, True)
    dev = lambda t: [None if a is None else torch.from_numpy(a.copy()).to("cuda:0") for a in t]  # noqa: E731
    d_raw, d_m, d_v, d_g = dev(k.raw), dev(k.m), dev(k.v), dev(k.grads)
    got = model_step(ctx, d_raw, d_m, d_v, d_g, adam, want_grad_raw=True)
    for host, d in ((raw, d_raw), (m, d_m), (v, d_v)):
        for a, t in zip(host, d):
            assert same_bits(t.cpu().numpy(), a)
    assert same_bits(got["grad_raw"].cpu().numpy(), out["grad_raw"])
    assert got["params"].cpu().numpy().tobytes() == out["params"].tobytes()
    assert got["aabbs"].cpu().numpy().tobytes() == out["aabbs"].tobytes()
    for a, t in zip(out["act"][:4], got["act"][:4]):
        assert same_bits(t.cpu().numpy(), a)
    assert got["act"][4] is d_raw[4] and got["act"][5] is d_raw[5]
    # unaligned bases (views one float in): the dword paths, the same bits
    off = lambda t: [None if a is None else torch.cat([a.new_zeros(1), a.reshape(-1)])[1:].reshape(a.shape)  # noqa: E731
                     for a in t]
    o_raw, o_m, o_v, o_g = off(dev(k.raw)), off(dev(k.m)), off(dev(k.v)), off(dev(k.grads))
    assert o_raw[1].data_ptr() % 16 == 4
    got2 = model_step(ctx, o_raw, o_m, o_v, o_g, adam, want_grad_raw=True)
    for host, d in ((raw, o_raw), (m, o_m), (v, o_v)):
        for a, t in zip(host, d):
            assert same_bits(t.cpu().numpy(), a)
    assert got2["params"].cpu().numpy().tobytes() == out["params"].tobytes()


def scene_arrays(ctx, act):
    sc = gsrt.Scene.from_model(ctx, *act[:4])
    try:
        return sc.download()
    finally:
        sc.close()


@pytest.mark.parametrize("n", [n for n in SIZES if n])
def test_scene_arrays_are_the_scene_builds(ctx, n):
    k = R.case(n)
    a = gsrt.model_activate(ctx, k.raw)
    nq, q = R.normalise_f32(k.raw[1])
    assert u32(a["act"][1]).tobytes() == u32(q).tobytes() and u32(a["act"][0]).tobytes() == u32(k.raw[0]).tobytes()
    assert a["act"][4].tobytes() == k.raw[4].tobytes() and a["act"][4] is not k.raw[4]
    params, aabbs = scene_arrays(ctx, a["act"])
    assert a["params"].tobytes() == params.tobytes() and a["aabbs"].tobytes() == aabbs.tobytes()
    raw, m, v, adam, out = run_step(ctx, k, True)
    assert u32(out["act"][1]).tobytes() == u32(R.normalise_f32(raw[1])[1]).tobytes()
    assert same_bits(out["act"][0], raw[0]) and out["act"][4] is raw[4]
    params, aabbs = scene_arrays(ctx, out["act"])
    assert same_bits(out["params"], params) and same_bits(out["aabbs"], aabbs)
    # activate(raw') is the step's own output: one code path
    b = gsrt.model_activate(ctx, raw)
    assert same_bits(b["params"], out["params"]) and same_bits(b["aabbs"], out["aabbs"])
    if n >= 8:  # the zero quaternion: act.rot = 0 and R = I, Sigma = diag(s^2)
        z = k.zero_quat
        s = a["act"][2][z]
        assert not a["act"][1][z].any() and not a["params"][z, [5, 6, 8]].any()
        assert np.array_equal(a["params"][z, [4, 7, 9]], s * s)


def report(label, got, ref, M, N, require_reached=True):
    got64 = np.asarray(got, np.float64)
    assert got64.shape == ref.shape and np.isfinite(got64).all(), label
    err, bound = np.abs(got64 - ref), N * EPS * M
    reached = M > 0
    worst = float((err[reached] / bound[reached]).max()) if reached.any() else 0.0
    print(f"{label}: {int(reached.sum())} of {M.size} entries, N = {N}; worst error / (N 2^-24 M) = {worst:.3g}")
    rep = os.environ.get("COR_F64_REPORT")
    if rep:
        with open(rep, "a") as fh:
            fh.write(json.dumps({"case": label, "entries": int(M.size), "ops": N, "worst_ratio": worst}) + "\n")
    assert (err <= bound).all(), f"{label}: worst error / bound = {worst:.3g}"
    assert not require_reached or reached.sum() > M.size // 2, label
    return worst


def test_activations_and_chain_against_float64(ctx):
    k = R.case(300)
    raw, m, v, adam, out = run_step(ctx, k, False)
    a0 = gsrt.model_activate(ctx, k.raw)["act"]
    ref = R.activate_f64(*k.raw[1:4])
    report("model_step act.scale", a0[2], ref.s, ref.s, R.N_ACT["scale"])
    report("model_step act.opacity", a0[3], ref.o, ref.o, R.N_ACT["opacity"])
    report("model_step act.rot", a0[1], ref.q, np.abs(ref.q), 6)
    assert np.isfinite(k.grads[2][:, 5]).all()  # the NaN row's NaN is in slot 0, which the chain does not read
    c = R.chain_f64(k.raw[1], k.raw[2], k.raw[3], k.grads[1], k.grads[2][:, 5])
    graw = out["grad_raw"]
    report("model_step grad_raw rot", graw[:, 3:7], c.rot, c.M_rot, R.N_CHAIN["rot"])
    report("model_step grad_raw log scale", graw[:, 7:10], c.scale, c.M_scale, R.N_CHAIN["scale"])
    report("model_step grad_raw logit", graw[:, 10], c.opacity, c.M_opacity, R.N_CHAIN["opacity"])
    z = k.zero_quat
    assert not u32(graw[z, 3:7]).any() and not c.M_rot[z].any()  # +0 at the zero quaternion
    assert (c.M_rot[np.arange(300) != z] > 0).all()


def test_opacity_reset(ctx):
    rng = np.random.default_rng(9)
    for n in (1, 65, 1025):
        logit = rng.uniform(-8, 8, n).astype(np.float32)
        if n > 8:
            logit[3], logit[4], logit[5] = np.nan, np.inf, -np.inf
        m, v = rng.normal(0, 1, n).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
        limit = np.float32(np.log(0.01 / (1.0 - 0.01)))
        want = np.where(logit > limit, limit, logit).astype(np.float32)
        got = logit.copy()
        gsrt.model_opacity_reset(ctx, got, m, v, 0.01)
        assert same_bits(got, want) and not u32(m).any() and not u32(v).any()
        if n > 8:
            assert np.isnan(got[3]) and got[4] == limit and got[5] == -np.inf
        assert (got[np.isfinite(got)] <= limit).all()
        if n > 8:
            assert (got == logit).any() and (got[np.isfinite(logit)] != logit[np.isfinite(logit)]).any()  # some kept, some cut
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(gsrt.GsrtError) as e:
            gsrt.model_opacity_reset(ctx, got, m, v, bad)
        assert e.value.status == gsrt.E_ARG and "gsrt_model_opacity_reset" in str(e.value)


def test_deactivate_against_float64_and_round_trip(ctx):
    k = R.case(300, with_sh=True, channels=8)
    c0, r0, s0, o0, sh0 = S.scene()
    o = np.minimum(o0, np.float32(0.99))
    feat = k.raw[5]
    raw = gsrt.model_deactivate(ctx, (c0, r0, s0, o, sh0, feat))
    assert raw[0].tobytes() == c0.tobytes() and raw[1].tobytes() == r0.tobytes()
    assert raw[4].reshape(-1).tobytes() == sh0.tobytes() and raw[5].tobytes() == feat.tobytes()
    s64, o64 = s0.astype(np.float64), o.astype(np.float64)
    ls, lg = np.log(s64), np.log(o64 / (1 - o64))
    report("model_deactivate log scale", raw[2], ls, np.abs(ls) * R.E_LOG, 1, require_reached=False)
    report("model_deactivate logit", raw[3], lg, 2 + R.E_LOG * np.abs(lg), 1)
    # the round trip from the case's raw model
    act = gsrt.model_activate(ctx, k.raw)["act"]
    back = gsrt.model_deactivate(ctx, act)
    ref = R.activate_f64(*k.raw[1:4])
    ls, lg = k.raw[2].astype(np.float64), k.raw[3].astype(np.float64)
    report("round trip log scale", back[2], ls, R.E_EXP + R.E_LOG * np.abs(ls), 1)
    report("round trip logit", back[3], lg, (R.E_EXP + 2) / (1 - ref.o) + 2 + R.E_LOG * np.abs(lg), 1)
    assert back[0].tobytes() == k.raw[0].tobytes() and back[4].tobytes() == k.raw[4].tobytes()
    assert u32(back[1]).tobytes() == u32(R.normalise_f32(k.raw[1])[1]).tobytes()  # rot copied: the normalised one
    # opacity 1 and 0
    edge = gsrt.model_deactivate(ctx, (c0[:2], r0[:2], s0[:2], np.array([1.0, 0.0], np.float32)))
    assert edge[3].tolist() == [np.inf, -np.inf]


# ------------------------------------------------------------------------------------------------ 5: end to end
W, H, SPP, LAM = 48, 32, 4, 0.2
# one rate for the whole SH table: torch.optim.Adam below steps it as one tensor
RATES = dict(lr_center=2e-4, lr_rot=1e-3, lr_scale=2e-3, lr_opacity=2e-2, lr_sh_dc=2.5e-3, lr_sh_rest=2.5e-3)


def e2e_model():
    """the scene as a raw model, and a target rendered from a perturbed copy"""
    c, r, s, o, sh = S.scene()
    rng = np.random.default_rng(77)
    o = np.minimum(o, np.float32(0.99))
    c2 = (c + rng.normal(0, 0.01, c.shape)).astype(np.float32)
    s2 = (s * rng.uniform(0.9, 1.1, s.shape)).astype(np.float32)
    o2 = (o * rng.uniform(0.7, 1.0, o.shape)).astype(np.float32)
    sh2 = (sh + rng.normal(0, 0.05, sh.shape)).astype(np.float32)
    return (c, r, s, o, sh), (c2, r, s2, o2, sh2)


def test_end_to_end(ctx):
    import torch

    from gsrt.autograd import model_step, photometric_loss, render_model

    model, other = e2e_model()
    ubo = TG.camera(S.CASES[0])
    assert S.CASES[0] == ("origin", W, H, SPP)
    n = S.N
    sc_t = gsrt.Scene.from_model(ctx, *other)
    sc_t.build_bvh()
    target = np.ascontiguousarray(sc_t.render(ubo)[0][..., :3])
    sc_t.close()
    raw_np = gsrt.model_deactivate(ctx, model)
    sc = gsrt.Scene.from_model(ctx, *model)
    try:
        sc.build_bvh()
        # real gradient tables, and the bit-exact statement on them
        rgba = sc.render(ubo)[0]
        loss0, gimg = gsrt.image_loss(ctx, rgba, target, LAM)
        rows = sc.splat_grad(ubo, gimg)
        d_c, d_cov = sc.model_grad(ubo, rows)
        d_sh = sc.sh_grad(ubo, gimg)
        grads = [np.ascontiguousarray(d_c), np.ascontiguousarray(d_cov), np.ascontiguousarray(rows),
                 np.ascontiguousarray(d_sh).reshape(n, 16, 3), None]
        seen = R.seen_rows(rows)
        assert 20 < seen.sum() and (~seen).sum() > 0
        k = R.Case()
        k.n, k.grads, k.seen = n, grads, seen
        k.raw = [a.copy() for a in raw_np[:5]] + [None]
        k.raw[4] = k.raw[4].reshape(n, 16, 3)
        k.m = [np.zeros_like(a) for a in k.raw[:5]] + [None]
        k.v = [np.zeros_like(a) for a in k.raw[:5]] + [None]
        for sparse in (False, True):
            raw, m, v = k.copies()
            adam = gsrt.adam_params(**RATES, step=1, sparse=sparse)
            out = gsrt.model_step(ctx, raw, m, v, grads, adam, want_grad_raw=True)
            want = R.step_ref(k.raw, k.m, k.v, out["grad_raw"], grads[3], None, adam, gsrt.adam_scalars(adam),
                              seen if sparse else None)
            for g3, w3 in zip((raw, m, v), want):
                for g, w in zip(g3[:5], w3[:5]):
                    assert same_bits(g, w)
            assert u32(out["grad_raw"][:, :3]).tobytes() == u32(grads[0]).tobytes()

        # ten steps of the torch-free loop
        dev = "cuda:0"
        t_raw = [torch.from_numpy(a.copy()).to(dev) for a in k.raw[:5]] + [None]
        t_m = [torch.zeros_like(t) for t in t_raw[:5]] + [None]
        t_v = [torch.zeros_like(t) for t in t_raw[:5]] + [None]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        t_rgba, t_gimg, t_rows, t_c, t_cov, t_sh, t_out = new(H, W, 4), new(H, W, 4), new(n, 8), new(n, 3), new(n, 6), new(n, 48), new(4)
        t_target = torch.from_numpy(target).to(dev)
        torch.cuda.synchronize()
        losses = []
        for t in range(1, 12):
            sc.render_async(ubo, d_rgba=t_rgba.data_ptr())
            gsrt.image_loss(ctx, t_rgba.data_ptr(), t_target.data_ptr(), LAM, width=W, height=H, target_channels=3,
                            d_out=t_out.data_ptr(), d_grad=t_gimg.data_ptr(), asynchronous=True)
            if t == 11:  # the loss after ten steps
                ctx.synchronize()
                losses.append(float(t_out[0].item()))
                break
            sc.splat_grad_async(ubo, t_gimg.data_ptr(), t_rows.data_ptr())
            sc.model_grad_async(ubo, t_rows.data_ptr(), t_c.data_ptr(), t_cov.data_ptr())
            sc.sh_grad_async(ubo, t_gimg.data_ptr(), t_sh.data_ptr())
            out = model_step(ctx, t_raw, t_m, t_v, (t_c, t_cov, t_rows, t_sh), gsrt.adam_params(**RATES, step=t, sparse=True))
            losses.append(float(t_out[0].item()))
            sc.update(params=out["params"].data_ptr(), aabbs=out["aabbs"].data_ptr())
            sc.refit_bvh()
            sc.set_sh(t_raw[4].data_ptr())
            ctx.synchronize()  # the update's copies have read `out` before torch may reuse its memory
        print("torch-free loop, loss per step:", " ".join(f"{x:.5f}" for x in losses))
        assert len(losses) == 11 and np.isfinite(losses).all()
        assert losses[0] == pytest.approx(loss0["loss"], rel=1e-5) and losses[-1] < losses[0]
    finally:
        sc.close()

    # the same ten steps with render_model + torch.optim.Adam, activations in torch
    sc = gsrt.Scene.from_model(ctx, *model)
    try:
        sc.build_bvh()
        p = [torch.from_numpy(a.copy()).to(dev).requires_grad_(True) for a in k.raw[:5]]
        opt = torch.optim.Adam([dict(params=[p[0]], lr=RATES["lr_center"]), dict(params=[p[1]], lr=RATES["lr_rot"]),
                                dict(params=[p[2]], lr=RATES["lr_scale"]), dict(params=[p[3]], lr=RATES["lr_opacity"]),
                                dict(params=[p[4]], lr=RATES["lr_sh_dc"])], betas=(0.9, 0.999), eps=1e-15)
        ref_losses = []
        for t in range(11):
            rgba = render_model(sc, ubo, p[0], torch.nn.functional.normalize(p[1], dim=1), torch.exp(p[2]),
                                torch.sigmoid(p[3]), p[4])
            loss = photometric_loss(ctx, rgba, t_target, LAM)
            ref_losses.append(float(loss.item()))
            if t == 10:
                break
            opt.zero_grad()
            loss.backward()
            opt.step()
        print("render_model + torch.optim.Adam, loss per step:", " ".join(f"{x:.5f}" for x in ref_losses))
        assert ref_losses[-1] < ref_losses[0] and ref_losses[0] == pytest.approx(losses[0], rel=1e-4)
    finally:
        sc.close()


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals_with_a_context(ctx):
    import torch

    c, r, s, o, sh = S.scene()
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        ubo = TG.camera(S.CASES[-1])
        before = sc.render(ubo)[0]
        k = R.case(64, with_sh=True, channels=8)
        adam = k.adam(gsrt)
        P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

        def call(raw, m, v, grads, act=None, params=None, aabbs=None, graw=None, fc=(8, 8, 8, 8)):
            s_raw, s_m, s_v = (gsrt.ModelArrays(*[P(a) if not isinstance(a, int) else a for a in t], f)
                               for t, f in zip((raw, m, v), fc))
            s_g = gsrt.ModelGrads(*[P(a) if not isinstance(a, int) else a for a in grads])
            s_a = None if act is None else gsrt.ModelArrays(*[P(a) for a in act], fc[3])
            return gsrt.lib.gsrt_model_step(ctx.handle, k.n, ctypes.byref(s_raw), ctypes.byref(s_m), ctypes.byref(s_v),
                                            ctypes.byref(s_g), ctypes.byref(adam), None if s_a is None else ctypes.byref(s_a),
                                            P(params), P(aabbs), P(graw))

        def refused(status):
            assert status == gsrt.E_ARG
            assert b"gsrt_model_step" in gsrt.lib.gsrt_last_error(ctx.handle)

        raw, m, v = k.copies()
        keep = k.copies()
        assert call(raw, m, v, k.grads) == gsrt.OK  # the call itself is sound
        raw, m, v = k.copies()
        refused(call(raw[:4] + [None, raw[5]], m, v, k.grads))                      # sh missing in raw only
        refused(call(raw, m[:5] + [None], v, k.grads, fc=(8, 0, 8, 8)))             # features missing in m only
        refused(call(raw, m, v, k.grads, fc=(8, 8, 5, 8)))                          # the channel count disagrees
        refused(call(raw, m, v, k.grads[:3] + [None, k.grads[4]]))                  # grads.sh missing
        act = [np.zeros_like(a) for a in raw]
        refused(call(raw, m, v, k.grads, act=act[:4] + [None, act[5]]))             # act without sh
        refused(call(raw, m, v, k.grads, act=act[:1] + [raw[1]] + act[2:]))         # act.rot is raw.rot: aliasing
        refused(call(raw, m, v, k.grads, graw=k.grads[0]))                          # grad_raw over grads.center
        refused(call(raw, m[:1] + [v[1]] + m[2:], v, k.grads))                      # m.rot is v.rot
        params = np.zeros((k.n, 12), np.float32)
        refused(call(raw, m, v, k.grads, params=params, aabbs=params))              # two outputs, one array
        d_rot = torch.from_numpy(raw[1].copy()).to("cuda:0")
        torch.cuda.synchronize()
        refused(call(raw[:1] + [d_rot.data_ptr()] + raw[2:], m, v, k.grads))        # host and device pointers mixed
        big = gsrt.lib.gsrt_model_step(ctx.handle, 0x80000000, *([ctypes.byref(gsrt.ModelArrays())] * 3),
                                       ctypes.byref(gsrt.ModelGrads()), ctypes.byref(adam), None, None, None, None)
        refused(big)                                                                # n above GSRT_MAX_GAUSSIANS
        bad = k.adam(gsrt)
        bad.step = 0
        with pytest.raises(gsrt.GsrtError) as e:
            gsrt.model_step(ctx, raw, m, v, k.grads, bad)
        assert e.value.status == gsrt.E_ARG and "adam.step" in str(e.value)
        # nothing was written by any refused call, and the context renders as before
        for got3, want3 in zip((raw, m, v), keep):
            for g, w in zip(got3, want3):
                assert g.tobytes() == w.tobytes()
        assert not any(a.any() for a in act) and not params.any()
        assert sc.render(ubo)[0].tobytes() == before.tobytes()
        # the async forms take device pointers only
        s_raw = gsrt.ModelArrays(*[P(a) for a in raw], 8)
        assert gsrt.lib.gsrt_model_activate_async(ctx.handle, k.n, ctypes.byref(s_raw), None, P(params), None) == gsrt.E_ARG
        assert b"gsrt_model_activate" in gsrt.lib.gsrt_last_error(ctx.handle)
    finally:
        sc.close()


def test_empty_model(ctx):
    k = R.case(0, with_sh=True, channels=8)
    out = gsrt.model_activate(ctx, k.raw)
    assert out["params"].shape == (0, 12) and out["aabbs"].shape == (0, 6)
