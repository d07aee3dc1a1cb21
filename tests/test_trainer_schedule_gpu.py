"""3DGS's schedule in the training session (gsrt.Trainer): the active SH degree and the screen-size prune, on a 64 x 64
frame of 500 Gaussians (1 spp), in the style of tests/test_trainer_gpu.py: every bit-exact statement is about ONE trainer,
between what it downloads and the library's single calls fed with those downloads (gradient frames sum with float atomics,
so two trainers do not agree to the bit after a step).

The model: centres in a slab 2.5 to 5 in front of the camera, scales 0.03 to 0.12: s / d <= 0.048, and with f = 55 px and
the off-axis terms of the Jacobian (|x| / d, |y| / d <= 0.6) the larger eigenvalue of V stays below 2 (1.72 (f s / d)^2 + 0.3)
= 25, a screen radius of at most 15 px, under 3DGS's 20; for the prune test Gaussian BIG is moved to the axis with scale 1.5 at depth 3
(radius about 85 px: it covers the frame)."""
import ctypes

import numpy as np
import pytest

import gsrt
from test_features_gpu import _d2h, u32

pytestmark = pytest.mark.gpu

N, W, H, LAM, BIG = 500, 64, 64, 0.2, 123
RATES = dict(lr_center=2e-4, lr_rot=1e-3, lr_scale=2e-3, lr_opacity=2e-2, lr_sh_dc=2.5e-3, lr_sh_rest=2.5e-3)
_SHARED = {}


def adam(step=0):
    return gsrt.adam_params(**RATES, step=step, sparse=True)


def setup(ctx):
    """model, ubo and the target (a frame of the model with other colours and larger scales), made once"""
    if not _SHARED:
        rng = np.random.default_rng(33)
        c = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.5, 1.5, N), rng.uniform(-5.0, -2.5, N)], 1).astype(np.float32)
        r = rng.normal(size=(N, 4))
        r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)
        s = np.exp(rng.uniform(np.log(0.03), np.log(0.12), (N, 3))).astype(np.float32)
        o = rng.uniform(0.3, 0.9, N).astype(np.float32)
        sh = rng.normal(0.0, 0.05, (N, 16, 3)).astype(np.float32)
        sh[:, 0, :] = rng.uniform(0.2, 1.5, (N, 3))
        ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 1, 16)
        sh_t = sh + rng.normal(0.0, 0.2, sh.shape).astype(np.float32)
        sc = gsrt.Scene.from_model(ctx, c, r, s * np.float32(1.2), o, sh_t)
        sc.build_bvh()
        target = np.ascontiguousarray(sc.render(ubo)[0][..., :3])
        sc.close()
        assert target.max() > 0.1
        _SHARED.update(model=(c, r, s, o, sh), ubo=ubo, target=target)
    return _SHARED["model"], _SHARED["ubo"], _SHARED["target"]


def tables(tr, n=N):
    st = tr.state()
    rd = lambda addr, w: _d2h(addr, (n, w) if w > 1 else (n,))  # noqa: E731
    out = {k: [rd(a, w) for a, w in zip(st[k], (3, 4, 3, 1, 48))] for k in ("raw", "m", "v")}
    out["grads"] = [rd(a, w) for a, w in zip(st["grads"], (3, 6, 8, 48))]
    out["stats"] = _d2h(st["stats"], (n, 2))
    out["radii"] = _d2h(tr.radii(), (n,))
    return out


def sh_words(t, which):
    return u32(t[which][4]).reshape(-1, 48)


def test_degree_zero_then_one(ctx):
    model, ubo, target = setup(ctx)
    with gsrt.Trainer(ctx, model) as tr:
        assert tr.sh_degree == 3
        tr.sh_degree = 0
        assert tr.sh_degree == 0
        before = tables(tr)
        for _ in range(3):
            tr.step(ubo, target, adam(), lam=LAM)
        after = tables(tr)
        for which in ("raw", "m", "v"):
            assert np.array_equal(sh_words(after, which)[:, 3:], sh_words(before, which)[:, 3:]), which
            changed = (sh_words(after, which)[:, :3] != sh_words(before, which)[:, :3]).any(1)
            assert changed.sum() > N // 8, which  # coefficient 0 moved (for the Gaussians the frames saw)
        assert not u32(after["m"][4]).reshape(-1, 48)[:, 3:].any()  # inactive moments are still +0
        assert (u32(after["raw"][0]) != u32(before["raw"][0])).any()
        # raising the degree: words 3..11 move, words 12.. do not
        tr.sh_degree = 1
        tr.step(ubo, target, adam(), lam=LAM)
        risen = tables(tr)
        for which in ("raw", "m", "v"):
            assert np.array_equal(sh_words(risen, which)[:, 12:], sh_words(before, which)[:, 12:]), which
            assert ((sh_words(risen, which)[:, 3:12] != sh_words(after, which)[:, 3:12]).any(1)).sum() > N // 8, which
        assert tr.info()["step"] == 4 and tr.sh_degree == 1
        # the scene shows the stepped rows
        raw, act = tr.download()
        assert np.array_equal(u32(raw[4]).reshape(-1, 48), sh_words(risen, "raw"))


def test_degree_three_is_the_composed_calls(ctx):
    """a step at the default degree: raw, m, v are gsrt.model_step's of the pre-step state and the trainer's own tables,
    and the statistics gsrt.density_stats_add's of its own rows, bit for bit; radii only where the statistic counted"""
    model, ubo, target = setup(ctx)
    with gsrt.Trainer(ctx, model) as tr:
        before = tables(tr)
        assert not u32(before["radii"]).any() and not u32(before["stats"]).any()
        for t in (1, 2):
            tr.step(ubo, target, adam(), lam=LAM)
            after = tables(tr)
            raw, m, v = ([a.copy() for a in before[k]] + [None] for k in ("raw", "m", "v"))
            gsrt.model_step(ctx, raw, m, v, after["grads"] + [None], adam(t))
            for k, want3 in (("raw", raw), ("m", m), ("v", v)):
                for name, g, w in zip(("center", "rot", "scale", "opacity", "sh"), after[k], want3):
                    assert u32(g).tobytes() == u32(w).tobytes(), (t, k, name)
            want_stats = gsrt.density_stats_add(ctx, after["grads"][2], before["stats"].copy(), W, H)
            assert u32(after["stats"]).tobytes() == u32(want_stats).tobytes()
            seen = (after["grads"][2][:, :6] != 0).any(1)
            assert seen.sum() > N // 8 and not u32(after["radii"])[~seen & (before["radii"] == 0)].any()
            assert (after["radii"][seen] >= 1).all() and (after["radii"] <= 20).all()
            assert (after["radii"] >= before["radii"]).all()
            before = after


def test_screen_prune_drops_the_frame_filling_gaussian(ctx):
    (c, r, s, o, sh), ubo, target = setup(ctx)
    c, s, o = c.copy(), s.copy(), o.copy()
    c[BIG], s[BIG], o[BIG] = (0.0, 0.0, -3.0), 1.5, 0.5
    model = (c, r, s, o, sh)
    P = gsrt.densify_params(float("inf"), 1.0, 0.0)  # nothing is densified, nothing pruned by opacity or scale
    with gsrt.Trainer(ctx, model) as tr, gsrt.Trainer(ctx, model) as twin:
        for t in (tr, twin):
            t.step(ubo, target, adam(), lam=LAM)
        pre, pre_twin = tables(tr), tables(twin)
        radii = pre["radii"]
        print(f"screen radius of the frame-filling Gaussian: {radii[BIG]:.0f} px; the others' largest: {np.delete(radii, BIG).max():.0f}")
        assert radii[BIG] > 20 and 70 <= radii[BIG] <= 100 and np.delete(radii, BIG).max() <= 20
        assert twin.densify(P, 5) == N and twin.info()["n"] == N
        assert tr.densify(P, 5, max_screen_radius=20.0) == N - 1 and tr.info()["n"] == N - 1
        # centres pass through a densify bit for bit: exactly BIG is gone, relative to the twin's plain densify
        assert u32(tables(twin)["raw"][0]).tobytes() == u32(pre_twin["raw"][0]).tobytes()
        post = tables(tr, N - 1)
        assert u32(post["raw"][0]).tobytes() == u32(np.delete(pre["raw"][0], BIG, axis=0)).tobytes()
        assert u32(post["m"][0]).tobytes() == u32(np.delete(pre["m"][0], BIG, axis=0)).tobytes()
        for t in (tr, twin):
            assert not u32(_d2h(t.radii(), (N,))).any() and not u32(_d2h(t.state()["stats"], (N, 2))).any()
        assert np.isfinite(tr.step(ubo, target, adam(), lam=LAM)["loss"])
        assert (_d2h(tr.radii(), (N - 1,)) <= 20).all()


def test_refusals(ctx):
    model, ubo, target = setup(ctx)
    with gsrt.Trainer(ctx, model) as tr:
        with pytest.raises(gsrt.GsrtError) as e:
            tr.sh_degree = 4
        assert e.value.status == gsrt.E_ARG and "sh_degree" in str(e.value) and tr.sh_degree == 3
        with pytest.raises(gsrt.GsrtError) as e:
            tr.densify(gsrt.densify_params(1.0, 1.0, 0.0), 0, max_screen_radius=float("nan"))
        assert e.value.status == gsrt.E_ARG and tr.info() == dict(n=N, capacity=N, step=0)
        assert gsrt.lib.gsrt_trainer_sh_degree(tr.handle, None) == gsrt.E_ARG
        assert gsrt.lib.gsrt_trainer_radii(tr.handle, None) == gsrt.E_ARG
    u = ctypes.c_uint32(7)
    assert gsrt.lib.gsrt_trainer_set_sh_degree(None, 0) == gsrt.E_ARG
    assert gsrt.lib.gsrt_trainer_sh_degree(None, ctypes.byref(u)) == gsrt.E_ARG and u.value == 7
    # without SH a degree is accepted and ignored
    with gsrt.Trainer(ctx, model[:4] + (None,)) as tr:
        tr.sh_degree = 0
        assert np.isfinite(tr.step(ubo, target, adam(), lam=LAM)["loss"])
