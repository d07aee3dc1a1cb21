"""The blocking forms that stage host arrays through one call-array list (gsrt_api_util.hpp: CallArray, run_staged):
gsrt_density_stats_add, gsrt_densify_count, gsrt_densify, gsrt_image_loss, gsrt_frame_loss, gsrt_normal_noise, the
gsrt_splat_*grad_to_model pair and gsrt_pose_grad, through the C ABI itself (the Python wrappers refuse mixtures first).

Host form against device form: the same inputs as numpy arrays and as torch tensors give the same bits. Kernel and launch
are the same and every one of these calls is documented as free of atomics (gsrt.h), so nothing about rounding is in play.
Sizes: n in {1, 65, 300} (a lane, past a 64-lane wave, past a 256-thread block), images 17 x 9 (no multiple of the loss
tile). What the existing GPU tests already hold (values against the references, the refusals of bad parameters) is not
repeated; here are the staging's own edges: partial downloads, mixed sides, a shared host region, empty calls."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import gsrt

pytestmark = pytest.mark.gpu

L = gsrt.lib
NS = [1, 65, 300]
W, H = 17, 9
FILL = np.float32(-7.25)  # what an output array holds before a call
DEV = "cuda:0"


def last(ctx):
    return L.gsrt_last_error(ctx.handle).decode()


class Arrays:
    """the same arrays on both sides: host(name) and dev(name) are addresses, the tensors stay alive with the object"""

    def __init__(self, **arrays):
        self.h = {k: np.ascontiguousarray(v).copy() for k, v in arrays.items()}
        self.d = {k: torch.from_numpy(v.copy()).to(DEV) for k, v in self.h.items()}
        torch.cuda.synchronize()

    def addr(self, name, dev):
        return self.d[name].data_ptr() if dev else self.h[name].ctypes.data

    def got(self, name, dev):
        return self.d[name].cpu().numpy() if dev else self.h[name]


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def model(n, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    rot = f(n, 4)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    centre = f(n, 3) * np.float32(0.8) + np.array([0, 0, -3], np.float32)
    return dict(center=centre, rot=rot, scale=rng.uniform(0.02, 0.2, (n, 3)).astype(np.float32),
                opacity=rng.uniform(0.05, 0.95, n).astype(np.float32), sh=f(n, 48))


# ------------------------------------------------------------------------------------------ density statistics, count
@pytest.mark.parametrize("n", NS)
def test_density_stats_add(ctx, n):
    rng = np.random.default_rng(n)
    rows = rng.normal(0, 1, (n, 8)).astype(np.float32)
    rows[1::3] = 0  # not seen
    stats = rng.uniform(0, 4, (n, 2)).astype(np.float32)
    a = Arrays(rows=rows, stats=stats)
    for dev in (False, True):
        assert L.gsrt_density_stats_add(ctx.handle, n, W, H, a.addr("rows", dev), a.addr("stats", dev)) == gsrt.OK, last(ctx)
    assert same(a.got("stats", False), a.got("stats", True))
    assert (a.h["stats"][0] > stats[0]).all() and same(a.h["stats"][1::3], stats[1::3])  # added to where seen, only there
    assert same(a.got("rows", False), rows)


def count_inputs(n):
    m = model(n, 10 + n)
    rng = np.random.default_rng(20 + n)
    stats = np.stack([rng.uniform(0, 2, n), np.ones(n)], 1).astype(np.float32)
    return m, stats, gsrt.densify_params(1.0, float(np.median(m["scale"].max(1))), 0.3)


@pytest.mark.parametrize("n", NS)
def test_densify_count_every_mixture(ctx, n):
    m, stats, P = count_inputs(n)
    a = Arrays(scale=m["scale"], opacity=m["opacity"], stats=stats)
    got = {}
    for sides in itertools.product((False, True), repeat=3):
        out = ctypes.c_uint32(0xFFFFFFFF)
        st = L.gsrt_densify_count(ctx.handle, n, a.addr("scale", sides[0]), a.addr("opacity", sides[1]),
                                  a.addr("stats", sides[2]), ctypes.byref(P), ctypes.byref(out))
        assert st == gsrt.OK, (sides, last(ctx))
        got[sides] = out.value
    assert len(set(got.values())) == 1 and got[(True, True, True)] <= 2 * n, got


# ------------------------------------------------------------------------------------------ densify
FIELDS = (("center", 3), ("rot", 4), ("scale", 3), ("opacity", 1), ("sh", 48))


def densify_call(ctx, n, ins, stats, noise, P, outs, origin, cap, dev):
    a_in = gsrt.ModelArrays(*[ins.addr(k, dev) for k, _ in FIELDS], None, 0)
    a_out = gsrt.ModelArrays(*[outs.addr(k, dev) for k, _ in FIELDS], None, 0)
    got = ctypes.c_uint32(0)
    st = L.gsrt_densify(ctx.handle, ctypes.byref(a_in), n, ins.addr(stats, dev), ins.addr(noise, dev), ctypes.byref(P),
                        ctypes.byref(a_out), outs.addr(origin, dev), cap, ctypes.byref(got))
    return st, got.value


def densify_arrays(n, cap):
    m, stats, P = count_inputs(n)
    noise = np.random.default_rng(30 + n).normal(0, 1, (n, 2, 3)).astype(np.float32)
    ins = Arrays(stats=stats, noise=noise, **m)
    outs = Arrays(origin=np.full(cap, 0x55555555, np.int32),
                  **{k: np.full((cap, w) if w > 1 else (cap,), FILL) for k, w in FIELDS})
    return ins, outs, P


@pytest.mark.parametrize("n", NS)
def test_densify_partial_rows(ctx, n):
    """n_out < cap: the host form downloads n_out rows of each output and of origin, the rest stays as it was"""
    m, stats, P = count_inputs(n)
    rows = gsrt.densify_count(ctx, m["scale"], m["opacity"], stats, P)
    cap = rows + 5
    ins, outs, P = densify_arrays(n, cap)
    for dev in (False, True):
        st, k = densify_call(ctx, n, ins, "stats", "noise", P, outs, "origin", cap, dev)
        assert st == gsrt.OK and k == rows, (dev, st, k, last(ctx))
    assert n < 65 or (outs.h["origin"][:rows] < 0).any()  # something was cloned or split
    for name in [k for k, _ in FIELDS] + ["origin"]:
        host, dev = outs.got(name, False), outs.got(name, True)
        assert same(host[:rows], dev[:rows]), name
        fill = np.int32(0x55555555) if name == "origin" else FILL
        assert (host[rows:] == fill).all() and (rows == 0 or not (host[:rows] == fill).all()), name


def test_densify_over_cap_writes_nothing(ctx):
    n = 300
    m, stats, P = count_inputs(n)
    rows = gsrt.densify_count(ctx, m["scale"], m["opacity"], stats, P)
    cap = rows - 1
    ins, outs, P = densify_arrays(n, cap)
    for dev in (False, True):
        st, k = densify_call(ctx, n, ins, "stats", "noise", P, outs, "origin", cap, dev)
        assert st == gsrt.E_ARG and k == rows, (dev, st, k)
        assert f"{rows} output rows needed, cap is {cap}" in last(ctx)
    for name, _ in FIELDS:
        assert (outs.got(name, False) == FILL).all(), name
    assert (outs.got("origin", False) == 0x55555555).all()


# ------------------------------------------------------------------------------------------ the losses
def frame(seed, channels):
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(0, 1, s).astype(np.float32)  # noqa: E731
    depth = u(H, W) * 4
    tdepth = u(H, W) * 4
    tdepth[::4, ::3] = 0  # no sample there
    return dict(rgba=u(H, W, 4), target=u(H, W, channels), mask=u(H, W), depth=depth, tdepth=tdepth,
                gimg=np.full((H, W, 4), FILL), gdepth=np.full((H, W), FILL))


@pytest.mark.parametrize("channels", [3, 4])
def test_image_loss(ctx, channels):
    a = Arrays(**frame(channels, channels))
    out = {}
    for dev in (False, True):
        out[dev] = np.full(4, FILL)
        st = L.gsrt_image_loss(ctx.handle, W, H, a.addr("rgba", dev), a.addr("target", dev), channels, 0.2,
                               out[dev].ctypes.data, a.addr("gimg", dev))
        assert st == gsrt.OK, (dev, last(ctx))
    assert same(out[False], out[True]) and np.isfinite(out[False]).all() and out[False][0] > 0
    assert same(a.got("gimg", False), a.got("gimg", True)) and not (a.h["gimg"] == FILL).any()


@pytest.mark.parametrize("full", [True, False], ids=["mask-depth-gradients", "bare"])
def test_frame_loss(ctx, full):
    a = Arrays(**frame(7, 3))
    P = gsrt.frame_loss_params(0.2, (0.25, 0.5, 1.0), 0.5) if full else gsrt.frame_loss_params()
    opt = lambda name, dev: a.addr(name, dev) if full else None  # noqa: E731
    out = {}
    for dev in (False, True):
        out[dev] = np.full(gsrt.FRAME_LOSS_SCALARS, FILL)
        st = L.gsrt_frame_loss(ctx.handle, W, H, a.addr("rgba", dev), a.addr("target", dev), 3, opt("mask", dev),
                               opt("depth", dev), opt("tdepth", dev), ctypes.byref(P), out[dev].ctypes.data,
                               opt("gimg", dev), opt("gdepth", dev))
        assert st == gsrt.OK, (dev, last(ctx))
    assert same(out[False], out[True]) and np.isfinite(out[False]).all() and out[False][0] > 0
    for name in ("gimg", "gdepth"):
        assert same(a.got(name, False), a.got(name, True)), name
        assert (a.h[name] == FILL).any() != full, name  # written in full, or not touched at all
    assert not full or out[False][5] > 0  # depth samples


# ------------------------------------------------------------------------------------------ normal noise
@pytest.mark.parametrize("count", NS)
def test_normal_noise(ctx, count):
    a = Arrays(out=np.full(count + 3, FILL))
    for dev in (False, True):
        assert L.gsrt_normal_noise(ctx.handle, count, 11, 2, a.addr("out", dev)) == gsrt.OK, last(ctx)
    host, dev = a.got("out", False), a.got("out", True)
    assert same(host, dev) and (host[count:] == FILL).all() and not (host[:count] == FILL).any()


# ------------------------------------------------------------------------------------------ the projection's backward
@pytest.fixture(scope="module", params=NS)
def scene(ctx, request):
    n = request.param
    m = model(n, 40 + n)
    sc = gsrt.Scene.from_model(ctx, m["center"], m["rot"], m["scale"], m["opacity"])
    sc.build_bvh()
    ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 1, 16)
    rows = np.random.default_rng(50 + n).normal(0, 1, (n, 8)).astype(np.float32)
    yield sc, ubo, n, rows
    sc.close()


@pytest.mark.parametrize("depth", [False, True], ids=["plain", "depth"])
def test_model_grad_every_mixture(ctx, scene, depth):
    sc, ubo, n, rows = scene
    fn = L.gsrt_splat_depth_grad_to_model if depth else L.gsrt_splat_grad_to_model
    got = {}
    for sides in itertools.product((False, True), repeat=3):
        a = Arrays(rows=rows, gc=np.full((n, 3), FILL), gv=np.full((n, 6), FILL))
        st = fn(sc.handle, gsrt._p(ubo), a.addr("rows", sides[0]), a.addr("gc", sides[1]), a.addr("gv", sides[2]), 0)
        assert st == gsrt.OK, (sides, last(ctx))
        got[sides] = (a.got("gc", sides[1]), a.got("gv", sides[2]))
        assert same(a.got("rows", sides[0]), rows)
    want = got[(True, True, True)]
    assert not (want[0] == FILL).any() and not (want[1] == FILL).any()
    for sides, (gc, gv) in got.items():
        assert same(gc, want[0]) and same(gv, want[1]), sides
    # accumulate adds to tables that are on the device: a host table is refused and stays as it was
    for sides in ((True, False, True), (True, True, False), (False, False, False)):
        a = Arrays(rows=rows, gc=np.full((n, 3), FILL), gv=np.full((n, 6), FILL))
        st = fn(sc.handle, gsrt._p(ubo), a.addr("rows", sides[0]), a.addr("gc", sides[1]), a.addr("gv", sides[2]), 1)
        assert st == gsrt.E_ARG and "accumulate needs device tables" in last(ctx), sides
        assert (a.got("gc", sides[1]) == FILL).all() and (a.got("gv", sides[2]) == FILL).all()


@pytest.mark.parametrize("depth", [False, True], ids=["plain", "depth"])
def test_pose_grad_both_sides(ctx, scene, depth):
    sc, ubo, n, rows = scene
    a = Arrays(rows=rows)
    out = {}
    for dev in (False, True):
        out[dev] = np.full(16, FILL)
        st = L.gsrt_pose_grad(sc.handle, gsrt._p(ubo), a.addr("rows", dev), int(depth), out[dev].ctypes.data)
        assert st == gsrt.OK, (dev, last(ctx))
    assert same(out[False], out[True]) and not (out[False] == FILL).any()
    d_out = torch.zeros(16, device=DEV)
    assert L.gsrt_pose_grad(sc.handle, gsrt._p(ubo), a.addr("rows", False), int(depth), d_out.data_ptr()) == gsrt.E_ARG
    assert "grad_model_view is a host pointer" in last(ctx)


# ------------------------------------------------------------------------------------------ all on one side, or refused
def test_one_mixed_tuple_each(ctx):
    n = 65
    ins, outs, P = densify_arrays(n, 2 * n)
    refused = lambda st: st == gsrt.E_ARG and "all be host pointers or all be device pointers" in last(ctx)  # noqa: E731
    assert refused(L.gsrt_density_stats_add(ctx.handle, n, W, H, ins.addr("noise", False), ins.addr("stats", True)))
    a_in = gsrt.ModelArrays(*[ins.addr(k, k == "scale") for k, _ in FIELDS], None, 0)
    a_out = gsrt.ModelArrays(*[outs.addr(k, False) for k, _ in FIELDS], None, 0)
    got = ctypes.c_uint32(0)
    assert refused(L.gsrt_densify(ctx.handle, ctypes.byref(a_in), n, ins.addr("stats", False), ins.addr("noise", False),
                                  ctypes.byref(P), ctypes.byref(a_out), outs.addr("origin", False), 2 * n, ctypes.byref(got)))
    f = Arrays(**frame(3, 3))
    out = np.full(gsrt.FRAME_LOSS_SCALARS, FILL)
    assert refused(L.gsrt_image_loss(ctx.handle, W, H, f.addr("rgba", False), f.addr("target", True), 3, 0.2, out.ctypes.data,
                                     f.addr("gimg", False)))
    FP = gsrt.frame_loss_params()
    assert refused(L.gsrt_frame_loss(ctx.handle, W, H, f.addr("rgba", False), f.addr("target", False), 3, f.addr("mask", True),
                                     None, None, ctypes.byref(FP), out.ctypes.data, f.addr("gimg", False), None))
    o = Arrays(logit=np.zeros(n, np.float32), m=np.ones(n, np.float32), v=np.ones(n, np.float32))
    assert refused(L.gsrt_model_opacity_reset(ctx.handle, n, o.addr("logit", False), o.addr("m", True), o.addr("v", False), 0.01))
    # nothing was written
    assert (out == FILL).all() and (f.h["gimg"] == FILL).all() and (outs.h["center"] == FILL).all() and (o.h["v"] == 1).all()


# ------------------------------------------------------------------------------------------ one host array in two slots
@pytest.mark.parametrize("n", NS)
def test_activate_with_shared_sh(ctx, n):
    """act.sh is raw.sh, one host array: the two slots share one staged region, and the rows come back as they were"""
    m = model(n, 60 + n)
    raw = [np.ascontiguousarray(x) for x in gsrt.model_deactivate(ctx, (m["center"], m["rot"], m["scale"], m["opacity"], m["sh"]))[:5]]
    want = gsrt.model_activate(ctx, tuple(raw))["act"]
    sh = raw[4].copy()
    act = [np.full_like(x, FILL) for x in raw[:4]]
    s_raw = gsrt.ModelArrays(*[x.ctypes.data for x in raw[:4]], sh.ctypes.data, None, 0)
    s_act = gsrt.ModelArrays(*[x.ctypes.data for x in act], sh.ctypes.data, None, 0)
    st = L.gsrt_model_activate(ctx.handle, n, ctypes.byref(s_raw), ctypes.byref(s_act), None, None)
    assert st == gsrt.OK, last(ctx)
    for got, ref in zip(act, want[:4]):
        assert same(got, np.asarray(ref, np.float32).reshape(got.shape))
    assert same(sh, raw[4])


# ------------------------------------------------------------------------------------------ empty calls
def test_empty_calls_touch_nothing(ctx):
    ins, outs, P = densify_arrays(4, 4)
    before = [{k: v.copy() for k, v in side.h.items()} for side in (ins, outs)]
    assert L.gsrt_density_stats_add(ctx.handle, 0, W, H, ins.addr("noise", False), ins.addr("stats", False)) == gsrt.OK
    out = ctypes.c_uint32(0)
    assert L.gsrt_densify_count(ctx.handle, 0, ins.addr("scale", False), ins.addr("opacity", False), ins.addr("stats", False),
                                ctypes.byref(P), ctypes.byref(out)) == gsrt.OK and out.value == 0
    for dev in (False, True):
        assert densify_call(ctx, 0, ins, "stats", "noise", P, outs, "origin", 4, dev) == (gsrt.OK, 0)
        assert L.gsrt_normal_noise(ctx.handle, 0, 1, 0, outs.addr("center", dev)) == gsrt.OK
    for side, was in zip((ins, outs), before):
        for k, v in was.items():
            assert same(side.got(k, False), v) and same(side.got(k, True), v), k
