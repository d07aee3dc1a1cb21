"""Adaptive density control on the GPU (gsrt_density_stats_add, gsrt_densify_count, gsrt_densify, gsrt_scene_from_model
with device sources, gsrt.autograd.densify / remap_state / render_model(density_stats=)) against the numpy reference of
tests/densify_ref.py, bit for bit: every output array, origin and n_out. The reference and the inputs are checked on the
CPU in tests/test_densify_ref.py (every decision occurs at least 10 times on the 300-Gaussian model).

Sizes and the level of the ordered sum each one crosses (256-lane workgroups of four waves; one workgroup scans the
workgroup totals, each of its 256 threads a run of ceil(workgroups / 256) consecutive totals):
    0            nothing runs but the scan, which writes n_out = 0
    1, 63, 64    one wave, partly and wholly filled
    65           a second wave: the wave totals in LDS
    300          a second workgroup: the scanned workgroup totals
    1025         five workgroups, the last with one Gaussian
    70 001       274 workgroups: every scanning thread sums a run of two totals, the last runs are empty
"""
import ctypes

import numpy as np
import pytest

import densify_ref as D
import gsrt
import test_geom_grad_gpu as TGG
import test_grad_f64 as S
import test_grad_f64_gpu as TG

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 300, 1025, 70001]
FIELDS = ("center", "rot", "scale", "opacity", "sh", "features")


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu_params(P):
    return gsrt.densify_params(float(P.grad_threshold), float(P.split_scale), float(P.min_opacity), float(P.max_scale),
                               float(P.shrink))


def same_model(got, ref, with_sh, with_feat):
    """got: the 7-tuple of gsrt.densify (numpy arrays); ref: densify_ref's namespace with SH and features"""
    assert got[6].dtype == np.int32 and np.array_equal(got[6], ref.origin)
    for name, g in zip(FIELDS, got[:6]):
        want = getattr(ref, name)
        if (name == "sh" and not with_sh) or (name == "features" and not with_feat):
            assert g is None
            continue
        assert g.dtype == np.float32 and g.shape == want.shape, name
        assert np.array_equal(u32(g), u32(want)), name


@pytest.mark.parametrize("with_feat", [False, True], ids=["nofeat", "feat5"])
@pytest.mark.parametrize("with_sh", [False, True], ids=["nosh", "sh"])
@pytest.mark.parametrize("n", SIZES)
def test_densify_matches_reference(ctx, n, with_sh, with_feat):
    """host arrays through the blocking call; densify_count gives the same n_out"""
    (c, r, s, o, sh, feat), stats, noise, P, ref = D.case(n)
    params = gpu_params(P)
    assert gsrt.densify_count(ctx, s, o, stats, params) == ref.n_out
    got = gsrt.densify(ctx, c, r, s, o, sh if with_sh else None, stats, noise, params, feat if with_feat else None)
    assert got[0].shape[0] == ref.n_out
    same_model(got, ref, with_sh, with_feat)


@pytest.mark.parametrize("n", [1025, 70001])
def test_device_path_matches_reference(ctx, n):
    """device tensors through gsrt_densify_async (gsrt.autograd.densify): cap = 2 n, trimmed views"""
    import torch

    from gsrt.autograd import densify

    (c, r, s, o, sh, feat), stats, noise, P, ref = D.case(n)
    t = [torch.from_numpy(a).to("cuda:0") for a in (c, r, s, o, sh, stats, noise)]
    got = densify(ctx, *t, gpu_params(P), features=torch.from_numpy(feat).to("cuda:0"))
    assert got[4].shape[1:] == (16, 3) and got[6].dtype == torch.int32
    same_model([g.cpu().numpy() for g in got], ref, True, True)
    # the count alone, from device addresses
    assert gsrt.densify_count(ctx, t[2].data_ptr(), t[3].data_ptr(), t[5].data_ptr(), gpu_params(P), n=n) == ref.n_out


def clean_model():
    """the 300-Gaussian scene as it is (no NaN opacity), with its stats and noise"""
    c, r, s, o, sh = S.scene()
    stats, noise = D.synthetic_stats(S.N)
    return c, r, s, o, sh, stats, noise


def test_all_split_and_all_prune(ctx):
    c, r, s, o, sh, _, noise = clean_model()
    ones = np.ones((S.N, 2), np.float32)
    for P, rows in ((D.params(0.0, 0.0, 0.0, 0.0), 2 * S.N), (D.params(0.0, 0.0, 2.0, 0.0), 0)):
        ref = D.densify(c, r, s, o, sh, None, ones, noise, P)
        assert ref.n_out == rows
        got = gsrt.densify(ctx, c, r, s, o, sh, ones, noise, gpu_params(P))
        assert got[0].shape[0] == rows
        same_model(got, ref, True, False)
        assert (got[6] < 0).all()


def test_cap_too_small_writes_nothing(ctx):
    """cap = n_out - 1: GSRT_E_ARG, n_out reported, and the output buffers keep the pattern they were filled with, through
    the blocking call on device arrays and through the asynchronous one"""
    import torch

    (c, r, s, o, sh, feat), stats, noise, P, ref = D.case(1025)
    t = [torch.from_numpy(a).to("cuda:0") for a in (c, r, s, o, sh, feat, stats, noise)]
    cap = ref.n_out - 1
    out = [torch.full((cap, k), 123.0, dtype=torch.float32, device="cuda:0") for k in (3, 4, 3, 1, 48, D.FEATURE_CHANNELS)]
    origin = torch.full((cap,), 77, dtype=torch.int32, device="cuda:0")
    d_n = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    a_in = gsrt.ModelArrays(*[x.data_ptr() for x in t[:6]], D.FEATURE_CHANNELS)
    a_out = gsrt.ModelArrays(*[x.data_ptr() for x in out], D.FEATURE_CHANNELS)
    params = gpu_params(P)
    n_out = ctypes.c_uint32(0)
    args = (ctypes.byref(a_in), 1025, ctypes.c_void_p(t[6].data_ptr()), ctypes.c_void_p(t[7].data_ptr()),
            ctypes.byref(params), ctypes.byref(a_out), ctypes.c_void_p(origin.data_ptr()), cap)
    st = gsrt.lib.gsrt_densify(ctx.handle, *args, ctypes.byref(n_out))
    assert st == gsrt.E_ARG and n_out.value == ref.n_out
    assert str(ref.n_out) in gsrt.lib.gsrt_last_error(ctx.handle).decode()
    assert gsrt.lib.gsrt_densify_async(ctx.handle, *args, ctypes.c_void_p(d_n.data_ptr())) == gsrt.OK
    ctx.synchronize()
    assert int(d_n.item()) == ref.n_out
    assert all(bool((x == 123.0).all()) for x in out) and bool((origin == 77).all())
    # with room for every row the same buffers (one row more) take the result
    out = [torch.full((cap + 1, k), 123.0, dtype=torch.float32, device="cuda:0") for k in (3, 4, 3, 1, 48, D.FEATURE_CHANNELS)]
    torch.cuda.synchronize()
    got = gsrt.densify(ctx, *[x.data_ptr() for x in t[:5]], t[6].data_ptr(), t[7].data_ptr(), params, t[5].data_ptr(),
                       n=1025, feature_channels=D.FEATURE_CHANNELS, out=[x.data_ptr() for x in out],
                       origin=(org := torch.zeros((cap + 1,), dtype=torch.int32, device="cuda:0")).data_ptr(), cap=cap + 1)
    assert got == ref.n_out
    host = [x.cpu().numpy() for x in out]
    host[3] = host[3][:, 0]
    host[4] = host[4].reshape(-1, 16, 3)
    same_model(host + [org.cpu().numpy()], ref, True, True)


def test_refused_arguments(ctx):
    import torch

    (c, r, s, o, sh, feat), stats, noise, P, ref = D.case(64)
    bad = gpu_params(P)
    bad.reserved[1] = 1
    with pytest.raises(gsrt.GsrtError) as e:
        gsrt.densify(ctx, c, r, s, o, None, stats, noise, bad)
    assert e.value.status == gsrt.E_ARG and "reserved" in str(e.value)
    with pytest.raises(gsrt.GsrtError) as e:
        gsrt.densify_count(ctx, s, o, stats, gsrt.densify_params(0.5, 0.1, 0.1, 0.0, 0.0))
    assert e.value.status == gsrt.E_ARG and "shrink" in str(e.value)
    # an out array that is the in array; host inputs with a device output
    arrays = [np.zeros((128, k), np.float32) for k in (3, 4, 3, 1)]
    org = np.zeros(128, np.int32)
    n_out = ctypes.c_uint32(0)
    params = gpu_params(P)
    a_in = gsrt.ModelArrays(c.ctypes.data, r.ctypes.data, s.ctypes.data, o.ctypes.data, None, None, 0)
    a_out = gsrt.ModelArrays(arrays[0].ctypes.data, r.ctypes.data, arrays[2].ctypes.data, arrays[3].ctypes.data, None, None, 0)
    call = lambda ai, ao: gsrt.lib.gsrt_densify(ctx.handle, ctypes.byref(ai), 64, gsrt._p(stats), gsrt._p(noise),  # noqa: E731
                                                ctypes.byref(params), ctypes.byref(ao), gsrt._p(org), 128, ctypes.byref(n_out))
    assert call(a_in, a_out) == gsrt.E_ARG and "in place" in gsrt.lib.gsrt_last_error(ctx.handle).decode()
    d_c = torch.zeros((128, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    a_out = gsrt.ModelArrays(d_c.data_ptr(), arrays[1].ctypes.data, arrays[2].ctypes.data, arrays[3].ctypes.data, None, None, 0)
    assert call(a_in, a_out) == gsrt.E_ARG and "all be" in gsrt.lib.gsrt_last_error(ctx.handle).decode()
    a_out = gsrt.ModelArrays(*[a.ctypes.data for a in arrays], None, arrays[0].ctypes.data, 3)  # features in out only
    assert call(a_in, a_out) == gsrt.E_ARG and "agree" in gsrt.lib.gsrt_last_error(ctx.handle).decode()
    # the statistic: a host and a device pointer, a zero width
    rows, st = np.zeros((64, 8), np.float32), np.zeros((64, 2), np.float32)
    d_st = torch.zeros((64, 2), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    L = gsrt.lib
    assert L.gsrt_density_stats_add(ctx.handle, 64, 8, 8, gsrt._p(rows), ctypes.c_void_p(d_st.data_ptr())) == gsrt.E_ARG
    assert L.gsrt_density_stats_add(ctx.handle, 64, 0, 8, gsrt._p(rows), gsrt._p(st)) == gsrt.E_ARG
    assert L.gsrt_density_stats_add(ctx.handle, 64, 8, 0, gsrt._p(rows), gsrt._p(st)) == gsrt.E_ARG
    assert L.gsrt_density_stats_add(ctx.handle, 0x80000000, 8, 8, gsrt._p(rows), gsrt._p(st)) == gsrt.E_ARG


def test_density_stats_add_matches_numpy(ctx):
    """rows of ordinary values, zeros, -0, a NaN in one slot, values in slots 6 and 7 only; stats that start from ordinary
    values, -0 and NaN payloads; twice, from host arrays and from device arrays: bit for bit"""
    import torch

    n, W, H = 1025, 48, 32
    rng = np.random.default_rng(74)
    rows = rng.normal(0.0, 1e-3, (n, 8)).astype(np.float32)
    kind = rng.integers(0, 6, n)
    rows[kind == 0] = 0.0
    rows[kind == 1] = -0.0
    rows[kind == 2, :] = 0.0
    rows[kind == 2, 3] = np.nan
    rows[kind == 3, :6] = 0.0  # slots 6 and 7 alone: not seen
    rows[kind == 4, 1:] = 0.0
    rows[::97, 0] = np.nan
    start = rng.uniform(0.0, 3.0, (n, 2)).astype(np.float32)
    start[::5] = (-0.0, 0.0)
    start.view(np.uint32)[3::7, 0] = 0x7FC01234  # a NaN payload
    once = D.stats_add(rows, start, W, H)
    twice = D.stats_add(rows, once, W, H)
    unseen = (kind == 0) | (kind == 1) | (kind == 3)
    unseen[::97] = False
    assert unseen.sum() > 100 and np.array_equal(u32(twice[unseen]), u32(start[unseen]))
    assert not np.array_equal(u32(twice[~unseen]), u32(once[~unseen]))
    host = start.copy()
    assert gsrt.density_stats_add(ctx, rows, host, W, H) is host
    assert np.array_equal(u32(host), u32(once))
    gsrt.density_stats_add(ctx, rows, host, W, H)
    assert np.array_equal(u32(host), u32(twice))
    d_rows, d_stats = torch.from_numpy(rows).to("cuda:0"), torch.from_numpy(start).to("cuda:0")
    torch.cuda.synchronize()
    gsrt.density_stats_add(ctx, d_rows.data_ptr(), d_stats.data_ptr(), W, H, n=n)
    assert np.array_equal(u32(d_stats.cpu().numpy()), u32(once))
    gsrt.density_stats_add(ctx, d_rows.data_ptr(), d_stats.data_ptr(), W, H, n=n, asynchronous=True)
    ctx.synchronize()
    assert np.array_equal(u32(d_stats.cpu().numpy()), u32(twice))


def frame_of(ctx, make):
    sc = make()
    try:
        sc.build_bvh()
        return sc.render(TG.camera(S.CASES[0]), gsrt.MODE_COR)[0], sc.download()
    finally:
        sc.close()


def device_scene(ctx, tensors):
    """Scene.from_model_device of torch tensors (center, rot, scale, opacity, sh)"""
    import torch

    t = [x.contiguous() for x in tensors]
    torch.cuda.synchronize()
    return gsrt.Scene.from_model_device(ctx, int(t[0].shape[0]), *[x.data_ptr() for x in t])


def test_from_model_device_matches_from_model(ctx):
    import torch

    c, r, s, o, sh = S.scene()
    t = [torch.from_numpy(a).to("cuda:0") for a in (c, r, s, o, sh)]
    for with_sh in (True, False):
        want, (wp, wa) = frame_of(ctx, lambda: gsrt.Scene.from_model(ctx, c, r, s, o, sh if with_sh else None))
        got, (gp, ga) = frame_of(ctx, lambda: device_scene(ctx, t if with_sh else t[:4]))
        assert gp.tobytes() == wp.tobytes() and ga.tobytes() == wa.tobytes()
        assert got.tobytes() == want.tobytes() and want[..., 3].mean() > 0.5
    # host and device sources in one call
    mixed = gsrt.lib.gsrt_scene_from_model
    h = ctypes.c_void_p()
    assert mixed(ctx.handle, gsrt._p(c), ctypes.c_void_p(t[1].data_ptr()), gsrt._p(s), ctypes.c_void_p(t[3].data_ptr()),
                 gsrt._p(np.ascontiguousarray(sh)), S.N, ctypes.byref(h)) == gsrt.OK
    sc = gsrt.Scene(ctx, h)
    got, (gp, ga) = frame_of(ctx, lambda: sc)
    assert gp.tobytes() == wp.tobytes()


def test_identity_keeps_every_bit_and_the_frame(ctx):
    """grad_threshold = +inf, min_opacity = 0, max_scale = 0: n_out = n, every array bit-identical, and a scene built from
    the device outputs renders the original scene's 48x32 frame"""
    import torch

    from gsrt.autograd import densify

    c, r, s, o, sh, stats, noise = clean_model()
    t = [torch.from_numpy(a).to("cuda:0") for a in (c, r, s, o, sh, stats, noise)]
    got = densify(ctx, *t, gsrt.densify_params(float("inf"), 0.0, 0.0, 0.0))
    assert got[0].shape[0] == S.N and got[5] is None
    for g, want in zip(got[:5], (c, r, s, o, sh)):
        assert np.array_equal(u32(g.cpu().numpy()), u32(want))
    assert np.array_equal(got[6].cpu().numpy(), np.arange(S.N, dtype=np.int32))
    want, _ = frame_of(ctx, lambda: gsrt.Scene.from_model(ctx, c, r, s, o, sh))
    frame, _ = frame_of(ctx, lambda: device_scene(ctx, got[:5]))
    assert frame.tobytes() == want.tobytes()


def test_prune_only_frame(ctx):
    """prune at the median opacity, nothing densified: the rebuilt scene's frame is that of a scene built from the
    numpy-filtered arrays"""
    import torch

    from gsrt.autograd import densify

    c, r, s, o, sh, stats, noise = clean_model()
    cut = np.float32(np.quantile(o[o < 1.0], 0.5))
    keep = o >= cut
    assert 10 <= (~keep).sum() <= S.N - 10
    t = [torch.from_numpy(a).to("cuda:0") for a in (c, r, s, o, sh, stats, noise)]
    got = densify(ctx, *t, gsrt.densify_params(float("inf"), 0.0, float(cut), 0.0))
    assert got[0].shape[0] == keep.sum()
    assert np.array_equal(got[6].cpu().numpy(), np.nonzero(keep)[0].astype(np.int32))
    want, _ = frame_of(ctx, lambda: gsrt.Scene.from_model(ctx, c[keep], r[keep], s[keep], o[keep], sh[keep]))
    frame, _ = frame_of(ctx, lambda: device_scene(ctx, got[:5]))
    assert frame.tobytes() == want.tobytes()


def test_render_model_density_stats(ctx):
    """After backward, density_stats holds the statistic of the backward's own splat rows. The rows come from float atomic
    adds, so they are held as tests/test_geom_grad_gpu.py holds splat rows: within 1e-3 M of the float64 rows. The norm is
    1-Lipschitz in (gx, gy), so |sum - norm of the float64 row| <= 1e-3 (M_0 W / 2 + M_1 H / 2), which also covers the three
    float32 roundings of the norm (M bounds the value). The count is 1 where Scene.splat_grad's rows are seen, 0 elsewhere.
    A second backward accumulates; density_stats=None leaves the gradients what they were."""
    import torch

    from gsrt.autograd import render_model

    case = S.CASES[0]
    _, W, H, _ = case
    c, r, s, o, sh = S.scene()
    G, sg, _ = TGG.reference(case, True)
    ubo = TG.camera(case)
    d_G = torch.from_numpy(np.ascontiguousarray(G)).to("cuda:0")
    stats = torch.zeros((S.N, 2), dtype=torch.float32, device="cuda:0")
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    grads = []
    try:
        sc.build_bvh()
        rows = sc.splat_grad(ubo, G)
        for st in (stats, stats, None):
            t = {k: torch.from_numpy(a).to("cuda:0").requires_grad_(True) for k, a in dict(c=c, r=r, s=s, o=o, sh=sh).items()}
            rgba = render_model(sc, ubo, t["c"], t["r"], t["s"], t["o"], t["sh"], density_stats=st)
            (rgba * d_G).sum().backward()
            grads.append({k: v.grad.cpu().numpy() for k, v in t.items()})
            if st is stats and len(grads) == 1:
                first = stats.cpu().numpy()
    finally:
        sc.close()
    second = stats.cpu().numpy()
    ref = np.hypot(sg.rows[:, 0] * (W / 2), sg.rows[:, 1] * (H / 2))
    M = sg.M[:, 0] * (W / 2) + sg.M[:, 1] * (H / 2)
    TG.hold("density statistic", case, sg.near, first[:, 0], ref, M)
    seen = (rows[:, :6] != 0).any(axis=1)
    assert np.array_equal(first[:, 1], seen.astype(np.float32)) and 50 < seen.sum()
    assert not u32(first[~seen]).any()
    assert np.array_equal(second[:, 1], 2 * first[:, 1])
    assert (np.abs(second[:, 0].astype(np.float64) - 2 * ref) <= 2 * TG.TOL * M + 1e-30).all()
    # density_stats=None: the same gradients (two frames' float atomics: the bounds of test_render_model_backward)
    with_stats, without = grads[1], grads[2]
    TG.hold("render_model opacity, stats", case, sg.near, with_stats["o"], sg.rows[:, 5], sg.M[:, 5])
    TG.hold("render_model opacity, no stats", case, sg.near, without["o"], sg.rows[:, 5], sg.M[:, 5])
    import cor_f64 as F
    import cor_f64_geom as Q

    M2 = Q.model_chain(ubo, c.astype(np.float64), Q.cov6(F.covariance(r, s)), sg.M).M2_center
    tol = 2 * TG.TOL + 4 * TGG.CHAIN_OPS * (1 + 1.7) * TGG.EPS
    assert (np.abs(with_stats["c"].astype(np.float64) - without["c"]) <= tol * M2).all()
    assert all(np.isfinite(g).all() and g.any() for g in without.values())


def test_remap_state(ctx):
    import torch

    from gsrt.autograd import remap_state

    m = torch.arange(12, dtype=torch.float32, device="cuda:0").reshape(4, 3) + 1
    origin = torch.tensor([0, -1, 2, -3, -3, 3], dtype=torch.int32, device="cuda:0")
    got = remap_state(m, origin).cpu().numpy()
    want = np.zeros((6, 3), np.float32)
    want[[0, 2, 5]] = m.cpu().numpy()[[0, 2, 3]]
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert remap_state(m[:, 0], origin).shape == (6,)
    assert remap_state(m, origin[:0]).shape == (0, 3)
