"""The training session (gsrt.Trainer over gsrt_trainer_*) on the 48 x 32, 4 spp `origin` case of tests/test_grad_f64.py
with the model, target and rates of test_model_step_gpu.test_end_to_end.

Gradient frames sum with float atomics, so two trainers do not agree to the bit after a step: every bit-exact statement
below is about ONE trainer, between what it downloads and the host forms of the library's calls fed with those downloads.

1. The first step's scalars are gsrt.image_loss's of Scene.render of a scene built from the same model, bit for bit.
2. The gradient tables after one step against the float64 backward (cor_f64.gradients, cor_f64_geom.splat_gradients and
   model_chain) of the upstream gradient gsrt.image_loss returns, with test_grad_f64_gpu.hold (1e-3 M) for the rows and the
   SH table and test_geom_grad_gpu's CHAIN_OPS (1 + kappa) 2^-24 M2 for the chained tables.
3. The step: the host form of gsrt.model_step on the pre-step raw, m, v with the trainer's own tables is the trainer's
   post-step state, for steps 1 and 2.
4. After three steps the borrowed scene is the activation of the downloaded raw model, arrays and frame.
5. Ten steps lower the loss; the depth path runs.
6. Densify: the host form of gsrt.densify on the pre-densify download with gsrt.normal_noise(6 n, seed, stream_id = step)
   gives the trainer's new model: its raw download is gsrt.model_deactivate of that result and its activated download
   gsrt.model_activate of that raw model (the trainer keeps the raw model; centre and SH pass through both unchanged,
   the rotation through the first, and are compared with the densify result directly); m and v are the numpy gather; the
   statistics are zero.
   A trainer without room refuses and stays as it was.
7. Opacity reset. 8. Refusals leave the trainer as it was. 9. The gsrt_train CLI.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cor_f64 as F
import cor_f64_geom as Q
import gsrt
import test_grad_f64 as S
import test_grad_f64_gpu as TG
from test_features_gpu import _d2h, u32
from test_geom_grad_gpu import CHAIN_OPS, EPS
from test_model_step_gpu import H, LAM, RATES, W, e2e_model, same_bits

pytestmark = pytest.mark.gpu

CASE = S.CASES[0]
N = S.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "3dgs-raytrace_amd", "bin", "gsrt_train")
_SHARED = {}


def adam():
    return gsrt.adam_params(**RATES, step=0, sparse=True)  # .step is ignored: the trainer counts


def setup(ctx):
    """model, ubo, and the target frame (rendered once)"""
    if "target" not in _SHARED:
        assert CASE == ("origin", W, H, 4)
        model, other = e2e_model()
        ubo = TG.camera(CASE)
        sc = gsrt.Scene.from_model(ctx, *other)
        sc.build_bvh()
        rgba, depth = sc.render_depth(ubo)
        sc.close()
        _SHARED.update(model=model, ubo=ubo, target=np.ascontiguousarray(rgba[..., :3]), t_rgba=rgba, t_depth=depth)
    return _SHARED["model"], _SHARED["ubo"], _SHARED["target"]


def tables(tr, n=N):
    """the trainer's device state as numpy arrays"""
    st = tr.state()
    widths = (3, 4, 3, 1, 48)
    rd = lambda addr, w: _d2h(addr, (n, w) if w > 1 else (n,))  # noqa: E731
    out = {k: [rd(a, w) for a, w in zip(st[k], widths)] for k in ("raw", "m", "v")}
    out["grads"] = [rd(a, w) for a, w in zip(st["grads"], (3, 6, 8, 48))]
    out["stats"] = _d2h(st["stats"], (n, 2))
    return out


def bits_equal(a, b):
    return u32(a).tobytes() == u32(b).tobytes()


def test_first_step_is_image_loss_of_the_frame(ctx):
    model, ubo, target = setup(ctx)
    sc = gsrt.Scene.from_model(ctx, *model)
    sc.build_bvh()
    want, _ = gsrt.image_loss(ctx, sc.render(ubo)[0], target, LAM)
    sc.close()
    with gsrt.Trainer(ctx, model) as tr:
        assert tr.info() == dict(n=N, capacity=N, step=0)
        got = tr.step(ubo, target, adam(), lam=LAM)
        assert tr.info()["step"] == 1
    for k in ("loss", "l1", "ssim", "mse"):
        assert np.float32(got[k]).tobytes() == np.float32(want[k]).tobytes(), k
    assert got["depth_l1"] == 0.0 and got["depth_samples"] == 0.0


def test_gradient_tables_match_f64(ctx):
    model, ubo, target = setup(ctx)
    c, r, s, o, sh = model
    sc = gsrt.Scene.from_model(ctx, *model)
    sc.build_bvh()
    G = gsrt.image_loss(ctx, sc.render(ubo)[0], target, LAM)[1]
    params, _ = sc.download()
    sc.close()
    with gsrt.Trainer(ctx, model) as tr:
        tr.step(ubo, target, adam(), lam=LAM)
        g_center, g_cov, rows, g_sh = tables(tr)["grads"]
    ref = F.gradients(ubo, c, r, s, o, sh, G_rgba=G)
    sg = Q.splat_gradients(ubo, c, r, s, o, sh, G_rgba=G)
    assert sg.digest == ref.digest
    assert not u32(rows[:, 6:]).any()
    TG.hold("trainer splat rows", CASE, sg.near, rows[:, :6], sg.rows[:, :6], sg.M[:, :6])
    TG.hold("trainer sh table", CASE, ref.near, g_sh.reshape(N, 16, 3), ref.sh, ref.M_sh)
    # the chained tables against the float64 chain of the trainer's own rows and the scene's own float32 parameters
    chain = Q.model_chain(ubo, params[:, :3].astype(np.float64), params[:, 4:10].astype(np.float64), rows.astype(np.float64))
    for name, got, want, M2 in (("centre", g_center, chain.center, chain.M2_center), ("cov", g_cov, chain.cov, chain.M2_cov)):
        bound = CHAIN_OPS * (1.0 + chain.kappa[:, None]) * EPS * M2
        err = np.abs(got.astype(np.float64) - want)
        reached = M2 > 0
        ratio = float((err[reached] / bound[reached]).max())
        print(f"trainer grad_{name}: worst error / (N (1 + kappa) 2^-24 M2) = {ratio:.3g}")
        assert (err <= bound).all(), (name, ratio)
        assert reached.sum() > M2.size // 8


def test_step_is_the_host_model_step(ctx):
    model, ubo, target = setup(ctx)
    with gsrt.Trainer(ctx, model) as twin, gsrt.Trainer(ctx, model) as tr:
        before = tables(twin)  # a twin that has not stepped: raw = deactivate(model), m = v = 0
        assert bits_equal(before["raw"][2], gsrt.model_deactivate(ctx, model)[2])
        assert not any(u32(a).any() for a in before["m"] + before["v"])
        for t in (1, 2):
            tr.step(ubo, target, adam(), lam=LAM)
            after = tables(tr)
            raw, m, v = ([a.copy() for a in before[k]] + [None] for k in ("raw", "m", "v"))
            gsrt.model_step(ctx, raw, m, v, after["grads"] + [None], gsrt.adam_params(**RATES, step=t, sparse=True))
            for k, want3 in (("raw", raw), ("m", m), ("v", v)):
                for name, g, w in zip(("center", "rot", "scale", "opacity", "sh"), after[k], want3):
                    assert same_bits(g, w), (t, k, name)
            assert not bits_equal(after["raw"][0], before["raw"][0])  # and it moved
            down = tr.download()[0]
            assert all(bits_equal(a, b) for a, b in zip(down, after["raw"]))
            before = after
        assert tr.info()["step"] == 2


def test_scene_follows_the_model(ctx):
    model, ubo, target = setup(ctx)
    with gsrt.Trainer(ctx, model) as tr:
        for _ in range(3):
            tr.step(ubo, target, adam(), lam=LAM)
        raw, act = tr.download()
        sc = tr.scene()
        params, aabbs = sc.download()
        want = gsrt.model_activate(ctx, raw)
        assert bits_equal(params, want["params"]) and bits_equal(aabbs, want["aabbs"])
        for a, b in zip(act, want["act"][:5]):
            assert bits_equal(a, b)
        frame = sc.render(ubo)[0]
        fresh = gsrt.Scene.from_model(ctx, *act)
        fresh.build_bvh()
        assert frame.tobytes() == fresh.render(ubo)[0].tobytes() and frame[..., 3].max() > 0.1
        fresh.close()
        tr.rebuild_bvh()
        assert sc.render(ubo)[0].tobytes() == frame.tobytes()


def test_ten_steps_lower_the_loss_and_depth_runs(ctx):
    model, ubo, target = setup(ctx)
    with gsrt.Trainer(ctx, model) as tr:
        losses = [tr.step(ubo, target, adam(), lam=LAM)["loss"] for _ in range(11)]
        print("trainer, loss per step:", " ".join(f"{x:.5f}" for x in losses))
        assert np.isfinite(losses).all() and losses[10] < losses[0]
        a = _SHARED["t_rgba"][..., 3]
        t_depth = np.where(a > 0.05, _SHARED["t_depth"] / np.maximum(a, 1e-6), 0.0).astype(np.float32)  # normalised
        got = tr.step(ubo, target, adam(), target_depth=t_depth,
                      params=gsrt.frame_loss_params(LAM, depth_weight=0.1, alpha_min=0.05))
        assert got["depth_samples"] > 0 and np.isfinite(list(got.values())).all()
        assert tr.info()["step"] == 12 and np.isfinite(tr.step(ubo, target, adam(), lam=LAM)["loss"])


def classes(scale, opacity, stats, P):
    """gsrt_densify's decision in numpy (gsrt.h): counts of prune, clone, split, keep"""
    m = scale.max(1)
    mean = np.where(stats[:, 1] > 0, stats[:, 0] / np.maximum(stats[:, 1], 1), 0).astype(np.float32)
    prune = ~(opacity >= np.float32(P.min_opacity)) | ((P.max_scale > 0) & (m > np.float32(P.max_scale)))
    dens = ~prune & (mean >= np.float32(P.grad_threshold))
    split = dens & (m > np.float32(P.split_scale))
    return dict(prune=int(prune.sum()), clone=int((dens & ~split).sum()), split=int(split.sum()),
                keep=int((~prune & ~dens).sum()))


def thresholds(act, stats):
    mean = np.where(stats[:, 1] > 0, stats[:, 0] / np.maximum(stats[:, 1], 1), 0)
    seen = mean[mean > 0]
    assert seen.size > 20
    return gsrt.densify_params(float(np.quantile(seen, 0.5)), float(np.median(act[2].max(1))),
                               float(np.quantile(act[3], 0.05)))


def test_densify(ctx):
    model, ubo, target = setup(ctx)
    seed = 0x1234567890ABCDEF
    with gsrt.Trainer(ctx, model, capacity=2 * N) as tr:
        for _ in range(5):
            tr.step(ubo, target, adam(), lam=LAM)
        raw, act = tr.download()
        pre = tables(tr)
        P = thresholds(act, pre["stats"])
        k = classes(act[2], act[3], pre["stats"], P)
        assert k["clone"] >= 1 and k["split"] >= 1 and k["prune"] >= 1 and k["keep"] >= 1, k
        rows = k["keep"] + 2 * (k["clone"] + k["split"])
        assert gsrt.densify_count(ctx, act[2], act[3], pre["stats"], P) == rows
        old_scene = tr.scene()
        assert tr.densify(P, seed) == rows and tr.info() == dict(n=rows, capacity=2 * N, step=5)
        del old_scene
        # the host form on the pre-densify download, with the noise the trainer drew
        noise = gsrt.normal_noise(ctx, 6 * N, seed, stream_id=5).reshape(N, 2, 3)
        c2, r2, s2, o2, sh2, _, origin = gsrt.densify(ctx, *act, pre["stats"], noise, P)
        assert origin.size == rows
        want_raw = gsrt.model_deactivate(ctx, (c2, r2, s2, o2, sh2))
        want_act = gsrt.model_activate(ctx, want_raw)["act"]
        raw_n, act_n = tr.download()
        for name, g, w in zip(("center", "rot", "scale", "opacity", "sh"), raw_n, want_raw):
            assert same_bits(g, w), ("raw", name)
        for name, g, w in zip(("center", "rot", "scale", "opacity", "sh"), act_n, want_act):
            assert same_bits(g, w), ("act", name)
        assert bits_equal(act_n[0], c2) and bits_equal(raw_n[1], r2) and bits_equal(act_n[4], sh2)
        post = tables(tr, rows)
        for which in ("m", "v"):
            for g, a in zip(post[which], pre[which]):
                want = u32(a)[np.maximum(origin, 0)].copy()
                want[origin < 0] = 0
                assert u32(g).tobytes() == want.tobytes(), which
        assert any(u32(a).any() for a in post["m"])  # kept rows carried their moments over
        assert not u32(_d2h(tr.state()["stats"], (2 * N, 2))).any()
        params, _ = tr.scene().download()
        assert bits_equal(params, gsrt.model_activate(ctx, raw_n)["params"])
        for _ in range(2):
            assert np.isfinite(list(tr.step(ubo, target, adam(), lam=LAM).values())).all()
        assert tr.info()["step"] == 7

    # no room: capacity = n and a densify that would grow
    with gsrt.Trainer(ctx, model, capacity=N) as tr:
        for _ in range(5):
            tr.step(ubo, target, adam(), lam=LAM)
        raw, act = tr.download()
        pre = tables(tr)
        P = thresholds(act, pre["stats"])
        P.min_opacity = 0.0  # nothing is pruned: the model can only grow
        k = classes(act[2], act[3], pre["stats"], P)
        assert k["prune"] == 0 and k["clone"] + k["split"] >= 1
        with pytest.raises(gsrt.GsrtError) as e:
            tr.densify(P, seed)
        assert e.value.status == gsrt.E_ARG and "capacity" in str(e.value)
        assert tr.info() == dict(n=N, capacity=N, step=5)
        raw2, act2 = tr.download()
        post = tables(tr)
        assert all(bits_equal(a, b) for a, b in zip(raw + act, raw2 + act2))
        for which in ("m", "v", "stats"):
            assert all(bits_equal(a, b) for a, b in zip(pre[which], post[which]))
        assert np.isfinite(tr.step(ubo, target, adam(), lam=LAM)["loss"])


def test_opacity_reset(ctx):
    model, ubo, target = setup(ctx)
    with gsrt.Trainer(ctx, model) as tr:
        for _ in range(2):
            tr.step(ubo, target, adam(), lam=LAM)
        pre = tables(tr)
        assert u32(pre["m"][3]).any()
        tr.opacity_reset(0.3)
        post = tables(tr)
        logit, m, v = pre["raw"][3].copy(), pre["m"][3].copy(), pre["v"][3].copy()
        gsrt.model_opacity_reset(ctx, logit, m, v, 0.3)
        assert bits_equal(post["raw"][3], logit) and not u32(post["m"][3]).any() and not u32(post["v"][3]).any()
        assert not bits_equal(post["raw"][3], pre["raw"][3])
        for f in (0, 1, 2, 4):
            assert bits_equal(post["raw"][f], pre["raw"][f]) and bits_equal(post["m"][f], pre["m"][f])
        raw, act = tr.download()
        assert act[3].max() <= np.float32(0.3) * (1 + 1e-6)
        fresh = gsrt.Scene.from_model(ctx, *act)
        fresh.build_bvh()
        assert tr.scene().render(ubo)[0].tobytes() == fresh.render(ubo)[0].tobytes()  # the next frame reflects it
        fresh.close()
        with pytest.raises(gsrt.GsrtError) as e:
            tr.opacity_reset(1.0)
        assert e.value.status == gsrt.E_ARG


def test_refused_steps_change_nothing(ctx):
    model, ubo, target = setup(ctx)
    with gsrt.Trainer(ctx, model) as tr:
        tr.step(ubo, target, adam(), lam=LAM)
        raw, _ = tr.download()
        pre = tables(tr)
        no_samples, empty = ubo.copy(), ubo.copy()
        no_samples["samples"], empty["width"] = 0, 0
        bad_adam = adam()
        bad_adam.beta1 = 1.0
        bad_loss = gsrt.frame_loss_params(LAM)
        bad_loss.reserved = 1
        import torch
        d_mask = torch.ones(H, W, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        refusals = [
            lambda: tr.step(ubo, target, adam(), lam=1.5),                            # lam outside [0, 1]
            lambda: tr.step(ubo, target, adam(), lam=float("nan")),
            lambda: tr.step(ubo, target, adam(), target_channels=5),                  # not 3 or 4
            lambda: tr.step(no_samples, target, adam(), lam=LAM),                     # what a COR frame refuses
            lambda: tr.step(ubo, target, bad_adam, lam=LAM),                          # what gsrt_adam_scalars refuses
            lambda: tr.step(ubo, target, adam(), params=bad_loss),
            lambda: tr.step(ubo, target, adam(), params=gsrt.frame_loss_params(LAM, depth_weight=-1.0)),
            lambda: tr.step(ubo, target, adam(), mask=d_mask.data_ptr(), lam=LAM),    # host and device mixed
        ]
        for i, call in enumerate(refusals):
            with pytest.raises(gsrt.GsrtError) as e:
                call()
            assert e.value.status == gsrt.E_ARG and "gsrt_trainer_step" in str(e.value), i
        L = gsrt.lib.gsrt_trainer_step
        P, A = gsrt.frame_loss_params(LAM), adam()
        args = (ctypes.byref(P), ctypes.byref(A), None)
        assert L(tr.handle, empty.ctypes.data, 0, target.ctypes.data, 3, None, None, *args) == gsrt.E_ARG  # an empty frame
        assert L(tr.handle, None, 0, target.ctypes.data, 3, None, None, *args) == gsrt.E_ARG
        assert L(tr.handle, ubo.ctypes.data, 0, None, 3, None, None, *args) == gsrt.E_ARG
        assert L(tr.handle, ubo.ctypes.data, 0, target.ctypes.data, 3, None, None, None, ctypes.byref(A), None) == gsrt.E_ARG
        assert tr.info() == dict(n=N, capacity=N, step=1)
        post = tables(tr)
        assert all(bits_equal(a, b) for a, b in zip(raw, tr.download()[0]))
        for which in ("raw", "m", "v", "grads"):
            assert all(bits_equal(a, b) for a, b in zip(pre[which], post[which])), which
        assert bits_equal(pre["stats"], post["stats"])
        assert np.isfinite(tr.step(ubo, target, adam(), lam=LAM)["loss"]) and tr.info()["step"] == 2
    # creation
    c, r, s, o, sh = model
    for bad in (dict(capacity=N - 1), dict(capacity=0)):
        with pytest.raises(gsrt.GsrtError) as e:
            gsrt.Trainer(ctx, model, **bad)
        assert e.value.status == gsrt.E_ARG
    feat = gsrt.ModelArrays(*[a.ctypes.data for a in (c, r, s, o, sh)], c.ctypes.data, 3)
    h = ctypes.c_void_p()
    assert gsrt.lib.gsrt_trainer_create(ctx.handle, ctypes.byref(feat), N, N, ctypes.byref(h)) == gsrt.E_ARG and not h.value
    plain = gsrt.ModelArrays(*[a.ctypes.data for a in (c, r, s, o, sh)], None, 0)
    assert gsrt.lib.gsrt_trainer_create(ctx.handle, ctypes.byref(plain), 0, N, ctypes.byref(h)) == gsrt.E_ARG


def test_cli_trains_and_writes_a_ply(ctx, tmp_path):
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 16, 5, True)
    o = np.minimum(o, np.float32(0.9))
    raw = gsrt.model_deactivate(ctx, (c, r, s, o, sh))
    gsrt.ply_write(tmp_path / "in.ply", *raw[:5])
    (tmp_path / "view.camera").write_text("0 0 0  0 0 -1\n")
    ubo = gsrt.camera_from_file(tmp_path / "view.camera", 60.0, 16, 16, 1.0, 1, 16)
    sc = gsrt.Scene.from_model(ctx, c, r, s * np.float32(1.1), o, sh)
    sc.build_bvh()
    np.ascontiguousarray(sc.render(ubo)[0][..., :3]).tofile(tmp_path / "target.bin")
    sc.close()
    (tmp_path / "views.txt").write_text(f"{tmp_path / 'view.camera'} {tmp_path / 'target.bin'}\n")
    run = subprocess.run([TRAIN, "--ply", str(tmp_path / "in.ply"), "--views", str(tmp_path / "views.txt"), "--width", "16",
                          "--height", "16", "--fovy", "60", "--iters", "3", "--out", str(tmp_path / "out.ply")],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    line = run.stdout.strip().splitlines()[-1].split()
    assert line[0] == "3" and line[4] == "16" and all(np.isfinite(float(x)) for x in line[1:4])
    assert gsrt.ply_info(tmp_path / "out.ply") == {"n": 16, "sh_degree": 3}
    assert all(np.isfinite(a).all() for a in gsrt.ply_read(tmp_path / "out.ply"))
