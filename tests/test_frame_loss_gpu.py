"""The frame loss on the GPU (gsrt_frame_loss, gsrt_frame_loss_async, gsrt.frame_loss, gsrt.autograd.frame_loss) against the
numpy reference of tests/frame_loss_ref.py in float64. The reference is checked on the CPU in
tests/test_frame_loss_ref.py.

Shapes (W x H), for kernels with tiles of 32 x 16 pixels and a 5-pixel halo: 1 x 1; 5 x 7 (the window overhangs on every
side); 17 x 33 (three tile rows); 70 x 37 (halos cross two tile borders each way, so a halo pixel is composited and masked
with its own alpha and mask); 1 x 4097 (257 tiles: lane 0 of the scalar reduction takes a second tile's five sums).

Inputs follow test_image_loss_gpu.images: smooth fields plus noise, a flat block of two constants, a block scaled outside
[0, 1], a block where target == frame exactly, by fractions of the image so that every shape has them. Extended:
  alpha in [0.3, 1]; 1 on the block where target == frame, so that x' - y' = 0 exactly under every option; 0.001, below
    alpha_min, on a block; 0.5 on a block whose D = 0.5 t exactly (e = 0, sign(0) = 0); and, in the cases that read no
    alpha, NaNs, infinities and large values instead (not read);
  the target is the composited frame plus a step of +-[0.005, 0.08], so that no difference is near 0;
  a mask in [0.25, 1] with a block of zeros and a block of ones;
  a target depth z +- [0.01, 0.5] around the frame's z = D / alpha in [1, 4], with non-positive, infinite and NaN entries
    (no samples).
inputs() asserts on the float64 values that |x' - y'| > 1e-5 outside the blocks where it is exactly 0 (target == frame,
mask == 0) and |e| > 1e-3 on every depth sample outside the e = 0 block, with no pixel excluded: float32 flips no sign.

Tolerances, per case, derived as tests/test_image_loss_gpu.py derives them. Gradients: 8 max |ref32 - ref64| over
grad_image (alpha slot included) and over grad_depth separately, ref32 the reference run in float32 in the header's
operation order. ssim: 8 max |map32 - map64|. l1 and mse: 2^-20 relative. depth_l1: 8 |ref32 - ref64| of the scalar plus
2^-20 relative. depth_samples: exact. loss: (1 - lam) tol_l1 + lam tol_ssim + depth_weight tol_depth plus 2^-23 |loss|.
"""
import functools

import numpy as np
import pytest

import frame_loss_ref as F
import gsrt

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (5, 7), (17, 33), (70, 37), (1, 4097)]
BG = (1.0, 0.25, 0.5)
DEPTH_WEIGHT = 0.5
OPTIONS = {"none": (), "mask": ("mask",), "background": ("background",), "depth": ("depth",),
           "all": ("mask", "background", "depth")}
KEYS = ("loss", "l1", "ssim", "mse", "depth_l1", "depth_samples")


@functools.lru_cache(maxsize=None)
def inputs(W, H, channels, option):
    """(arrays, kw): arrays = dict(rgba, target, same, half), kw = the keyword arguments of the option set (mask, depth,
    target_depth, background, depth_weight), for gsrt.frame_loss and the reference alike"""
    on = OPTIONS[option]
    rng = np.random.default_rng(1000 * W + H)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    x = np.stack([0.5 + 0.4 * np.sin(0.11 * (c + 1) * xx + 0.5 * c) * np.cos(0.07 * (c + 2) * yy) for c in range(3)], -1)
    x = np.clip(x + rng.normal(0.0, 0.05, x.shape), 0.0, 1.0)
    step = rng.uniform(0.005, 0.08, x.shape) * rng.choice([-1.0, 1.0], x.shape)

    def block(fy0, fy1, fx0, fx1):  # at least one pixel, whatever the shape
        y0, x0 = int(fy0 * H), int(fx0 * W)
        sel = np.zeros((H, W), bool)
        sel[y0:max(y0 + 1, int(fy1 * H)), x0:max(x0 + 1, int(fx1 * W))] = True
        return sel
    flat, wide = block(0.55, 0.9, 0.05, 0.45), block(0.5, 1.0, 0.55, 1.0)
    same, low, half = block(0.1, 0.45, 0.1, 0.5), block(0.0, 0.3, 0.6, 0.8), block(0.3, 0.5, 0.6, 0.9)
    same &= ~flat & ~wide
    half &= ~same
    x[flat], step[flat] = (0.6, 0.3, 0.8), (-0.05, 0.05, -0.05)
    x[wide] = 1.6 * x[wide] - 0.3
    x = x.astype(np.float32)
    a = rng.uniform(0.3, 1.0, (H, W)).astype(np.float32)
    a[flat], a[low], a[half], a[same] = 0.75, 0.001, 0.5, 1.0
    kw = {}
    comp = x.astype(np.float64)
    if "background" in on:
        kw["background"] = BG
        comp = comp + (1.0 - a.astype(np.float64))[..., None] * np.array(BG)
    y = (comp + step).astype(np.float32)
    y[same] = x[same]
    m = np.ones((H, W))
    if "mask" in on:
        mask = rng.uniform(0.25, 1.0, (H, W)).astype(np.float32)
        mask[block(0.0, 0.2, 0.0, 0.6)] = 1.0
        mask[block(0.6, 0.8, 0.3, 0.7)] = 0.0
        kw["mask"], m = mask, mask.astype(np.float64)
    zero = same | (m == 0.0)
    diff = np.abs(m[..., None] * comp - m[..., None] * y.astype(np.float64))
    assert not diff[zero].any() and (diff[~zero] > 1e-5).all()
    if "depth" in on:
        z = rng.uniform(1.0, 4.0, (H, W))
        t = (z + rng.uniform(0.01, 0.5, (H, W)) * rng.choice([-1.0, 1.0], (H, W))).astype(np.float32)
        junk = np.array([0.0, -1.0, np.inf, np.nan, -np.inf], np.float32)
        t.reshape(-1)[3::7] = junk[np.arange(t.reshape(-1)[3::7].size) % junk.size]
        D = (z * a).astype(np.float32)
        t[half] = rng.uniform(1.0, 4.0, int(half.sum())).astype(np.float32)
        D[half] = np.float32(0.5) * t[half]
        kw.update(depth=D, target_depth=t, depth_weight=DEPTH_WEIGHT)
        sample = np.isfinite(t) & (t > 0) & (a >= np.float32(1.0 / 255.0))
        assert sample[half].all() and not sample[low & ~same & ~half].any() and 0 < sample.sum()
        e = np.abs(D[sample].astype(np.float64) / a[sample] - t[sample])
        assert not e[half[sample]].any() and (e[~half[sample]] > 1e-3).all()
    else:
        half = np.zeros((H, W), bool)
    if not ("background" in on or "depth" in on):  # alpha is not read
        a = rng.choice(np.array([1e30, -1e30, np.inf, -np.inf, np.nan, 7.0], np.float32), (H, W))
    rgba = np.concatenate([x, a[..., None]], -1)
    if channels == 4:
        y = np.concatenate([y, rng.choice(np.array([1e30, np.inf, np.nan, 7.0], np.float32), (H, W, 1))], -1)
    for v in [rgba, y, same, half] + [v for v in kw.values() if isinstance(v, np.ndarray)]:
        v.setflags(write=False)
    return dict(rgba=rgba, target=y, same=same, half=half), kw


@functools.lru_cache(maxsize=None)
def reference(W, H, channels, option, lam):
    A, kw = inputs(W, H, channels, option)
    return tuple(F.frame_loss(A["rgba"], A["target"], lam, dt, **kw) for dt in (np.float64, np.float32))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scalars(d):
    return np.array([d[k] for k in KEYS], np.float32)


def call(ctx, W, H, channels, option, lam=0.2, **over):
    A, kw = inputs(W, H, channels, option)
    return gsrt.frame_loss(ctx, A["rgba"], A["target"], lam=lam, **dict(kw, **over))


def ident(v):
    return f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("shape,option,channels,lam",
                         [(s, o, c, 0.2) for o in OPTIONS for c in (3, 4) for s in SHAPES] +
                         [(s, "all", 3, lam) for lam in (0.0, 1.0) for s in SHAPES], ids=ident)
def test_matches_reference(ctx, shape, option, channels, lam):
    W, H = shape
    A, kw = inputs(W, H, channels, option)
    r64, r32 = reference(W, H, channels, option, lam)
    out, grad, gdepth = call(ctx, W, H, channels, option, lam)
    assert grad.dtype == np.float32 and grad.shape == (H, W, 4)
    assert (gdepth is None) == ("depth" not in kw)
    dw = kw.get("depth_weight", 0.0)

    tol_g = 8.0 * float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max())
    err_g = float(np.abs(grad.astype(np.float64) - r64["grad"]).max())
    tol_s = 8.0 * float(np.abs(r32["map"].astype(np.float64) - r64["map"]).max())
    err_s = abs(out["ssim"] - r64["ssim"])
    tol_l1, tol_mse = 2.0 ** -20 * r64["l1"], 2.0 ** -20 * r64["mse"]
    tol_d = 8.0 * abs(r32["depth_l1"] - r64["depth_l1"]) + 2.0 ** -20 * r64["depth_l1"]
    err_d = abs(out["depth_l1"] - r64["depth_l1"])
    tol_loss = (1 - lam) * tol_l1 + lam * tol_s + dw * tol_d + 2.0 ** -23 * abs(r64["loss"])
    print(f"frame_loss {option} {W}x{H} c{channels} lam {lam}: grad err {err_g:.3e} bound {tol_g:.3e} max |grad| "
          f"{np.abs(r64['grad']).max():.3e}; ssim err {err_s:.3e} bound {tol_s:.3e}; l1 err {abs(out['l1'] - r64['l1']):.3e} "
          f"bound {tol_l1:.3e}; mse err {abs(out['mse'] - r64['mse']):.3e} bound {tol_mse:.3e}; depth_l1 err {err_d:.3e} "
          f"bound {tol_d:.3e}; samples {out['depth_samples']:.0f} of {r64['depth_samples']}; loss err "
          f"{abs(out['loss'] - r64['loss']):.3e} bound {tol_loss:.3e}")
    assert np.isfinite(grad).all()
    assert err_g <= tol_g
    if gdepth is not None:
        tol_gd = 8.0 * float(np.abs(r32["grad_depth"].astype(np.float64) - r64["grad_depth"]).max())
        err_gd = float(np.abs(gdepth.astype(np.float64) - r64["grad_depth"]).max())
        print(f"    grad_depth err {err_gd:.3e} bound {tol_gd:.3e} max {np.abs(r64['grad_depth']).max():.3e}")
        assert gdepth.dtype == np.float32 and gdepth.shape == (H, W) and np.isfinite(gdepth).all()
        assert err_gd <= tol_gd
        assert not bits(gdepth)[~r64["sample"]].any()  # +0 bitwise
        assert not gdepth[A["half"]].any()  # sign(0) = 0
    if "background" not in kw and "depth" not in kw:
        assert not bits(grad[..., 3]).any()  # +0 bitwise
    if lam == 0.0:
        assert not grad[A["same"]][:, :3].any()
    assert abs(out["l1"] - r64["l1"]) <= tol_l1
    assert abs(out["mse"] - r64["mse"]) <= tol_mse
    assert err_s <= tol_s
    assert err_d <= tol_d
    assert out["depth_samples"] == r64["depth_samples"]
    assert abs(out["loss"] - r64["loss"]) <= tol_loss


@pytest.mark.parametrize("shape,channels", [(s, 3) for s in SHAPES] + [((70, 37), 4)], ids=ident)
def test_no_option_has_image_loss_bits(ctx, shape, channels):
    """no mask, no background, no depth: gsrt.image_loss's scalars and gradient, NaN alphas included"""
    W, H = shape
    A, kw = inputs(W, H, channels, "none")
    assert not kw and (W * H < 35 or np.isnan(A["rgba"][..., 3]).any())
    want, gwant = gsrt.image_loss(ctx, A["rgba"], A["target"], 0.2)
    out, grad, gdepth = gsrt.frame_loss(ctx, A["rgba"], A["target"])
    assert gdepth is None
    assert np.array_equal(bits([out[k] for k in KEYS[:4]]), bits([want[k] for k in KEYS[:4]]))
    assert out["depth_l1"] == 0.0 and out["depth_samples"] == 0.0
    assert np.array_equal(bits(grad), bits(gwant))
    assert not bits(grad[..., 3]).any()
    # a depth with weight 0 and no sample: the same bits again, and every grad_depth word +0
    t = np.zeros((H, W), np.float32)
    A1, _ = inputs(W, H, channels, "background")  # finite alphas: depth reads alpha
    want1, gwant1 = gsrt.image_loss(ctx, A1["rgba"], A1["target"], 0.2)
    out1, grad1, gdepth1 = gsrt.frame_loss(ctx, A1["rgba"], A1["target"], depth=np.ones((H, W), np.float32), target_depth=t)
    assert np.array_equal(bits([out1[k] for k in KEYS[:4]]), bits([want1[k] for k in KEYS[:4]]))
    assert np.array_equal(bits(grad1), bits(gwant1)) and not bits(gdepth1).any()


@pytest.mark.parametrize("shape", [(5, 7), (70, 37)], ids=ident)
def test_mask_semantics(ctx, shape):
    W, H = shape
    A, kw = inputs(W, H, 3, "all")
    ones = np.ones((H, W), np.float32)
    a, ga, da = call(ctx, W, H, 3, "all", mask=ones)
    b, gb, db = call(ctx, W, H, 3, "all", mask=None)
    assert np.array_equal(bits(scalars(a)), bits(scalars(b)))
    assert np.array_equal(bits(ga), bits(gb)) and np.array_equal(bits(da), bits(db))
    out, grad, gdepth = call(ctx, W, H, 3, "all")
    off = kw["mask"] == 0.0
    assert off.any() and not (bits(grad)[off] & 0x7FFFFFFF).any()  # +-0 in all four words
    r64, _ = reference(W, H, 3, "all", 0.2)
    assert (~r64["sample"]).any() and not bits(gdepth)[~r64["sample"]].any()


@pytest.mark.parametrize("shape", [(5, 7), (70, 37)], ids=ident)
def test_deterministic_and_no_gradient(ctx, shape):
    W, H = shape
    a, ga, da = call(ctx, W, H, 3, "all")
    b, gb, db = call(ctx, W, H, 3, "all")
    c, gc, dc = call(ctx, W, H, 3, "all", want_grad=False)
    assert gc is None and dc is None
    assert np.array_equal(bits(scalars(a)), bits(scalars(b))) and np.array_equal(bits(scalars(a)), bits(scalars(c)))
    assert np.array_equal(bits(ga), bits(gb)) and np.array_equal(bits(da), bits(db))


@pytest.mark.parametrize("channels", [3, 4])
def test_device_pointers_match_host_pointers(ctx, channels):
    """device tensors through the blocking call and through gsrt_frame_loss_async: the bits of the host path"""
    import torch

    W, H = 70, 37
    A, kw = inputs(W, H, channels, "all")
    want, gwant, dwant = call(ctx, W, H, channels, "all")
    dev = lambda v: torch.from_numpy(np.array(v)).to("cuda:0")  # noqa: E731
    x, y, m, d, t = dev(A["rgba"]), dev(A["target"]), dev(kw["mask"]), dev(kw["depth"]), dev(kw["target_depth"])
    g = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda:0")
    gd = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    common = dict(mask=m.data_ptr(), depth=d.data_ptr(), target_depth=t.data_ptr(), background=BG,
                  depth_weight=DEPTH_WEIGHT, width=W, height=H, target_channels=channels, d_grad=g.data_ptr(),
                  d_grad_depth=gd.data_ptr())
    got = gsrt.frame_loss(ctx, x.data_ptr(), y.data_ptr(), **common)
    assert np.array_equal(bits(scalars(got)), bits(scalars(want)))
    assert np.array_equal(bits(g.cpu().numpy()), bits(gwant)) and np.array_equal(bits(gd.cpu().numpy()), bits(dwant))
    out = torch.zeros(6, dtype=torch.float32, device="cuda:0")
    g.fill_(7.0)
    gd.fill_(7.0)
    torch.cuda.synchronize()
    assert gsrt.frame_loss(ctx, x.data_ptr(), y.data_ptr(), d_out=out.data_ptr(), asynchronous=True, **common) is None
    ctx.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(scalars(want)))
    assert np.array_equal(bits(g.cpu().numpy()), bits(gwant)) and np.array_equal(bits(gd.cpu().numpy()), bits(dwant))


def test_library_refusals_leave_outputs_untouched(ctx):
    """the C call's own refusals (the wrapper's are tests/test_frame_loss_host.py's): E_ARG, named, nothing written"""
    import ctypes

    W, H = 5, 7
    A, kw = inputs(W, H, 3, "all")
    arr = {k: np.array(v) for k, v in dict(rgba=A["rgba"], target=A["target"], mask=kw["mask"], depth=kw["depth"],
                                           target_depth=kw["target_depth"]).items()}
    out, grad, gdepth = np.full(6, 3.0, np.float32), np.full((H, W, 4), 3.0, np.float32), np.full((H, W), 3.0, np.float32)
    P = lambda v: None if v is None else ctypes.c_void_p(v.ctypes.data)  # noqa: E731
    good = gsrt.frame_loss_params(0.2, BG, DEPTH_WEIGHT)
    base = dict(width=W, height=H, channels=3, params=good, out=out, grad=grad, gdepth=gdepth, **arr)

    def run(**over):
        a = dict(base, **over)
        return gsrt.lib.gsrt_frame_loss(ctx.handle, a["width"], a["height"], P(a["rgba"]), P(a["target"]), a["channels"],
                                        P(a["mask"]), P(a["depth"]), P(a["target_depth"]),
                                        None if a["params"] is None else ctypes.byref(a["params"]), P(a["out"]),
                                        P(a["grad"]), P(a["gdepth"]))
    assert run() == gsrt.OK
    out[:], grad[:], gdepth[:] = 3.0, 3.0, 3.0
    nan = float("nan")
    for over, word in [(dict(rgba=None), "NULL"), (dict(out=None), "NULL"), (dict(params=None), "params is NULL"),
                       (dict(width=0), "width"), (dict(height=32769), "width"), (dict(channels=2), "target_channels"),
                       (dict(params=gsrt.frame_loss_params(lam=1.5)), "lambda"),
                       (dict(params=gsrt.frame_loss_params(flags=2)), "flag"),
                       (dict(params=gsrt.frame_loss_params(reserved=7)), "reserved"),
                       (dict(params=gsrt.frame_loss_params(background=(nan, 0, 0))), "background"),
                       (dict(params=gsrt.frame_loss_params(depth_weight=-1.0)), "depth_weight"),
                       (dict(params=gsrt.frame_loss_params(depth_weight=nan)), "depth_weight"),
                       (dict(params=gsrt.frame_loss_params(alpha_min=0.0)), "alpha_min"),
                       (dict(params=gsrt.frame_loss_params(alpha_min=nan)), "alpha_min"),
                       (dict(depth=None), "target_depth"), (dict(target_depth=None), "target_depth"),
                       (dict(depth=None, target_depth=None), "grad_depth needs"), (dict(grad=None), "grad_depth needs"),
                       (dict(grad=arr["rgba"]), "overlaps"), (dict(gdepth=arr["mask"]), "overlaps"),
                       (dict(gdepth=grad.reshape(-1)[-W * H:]), "overlap")]:
        assert run(**over) == gsrt.E_ARG, over
        assert word in gsrt.lib.gsrt_last_error(ctx.handle).decode(), (over, gsrt.lib.gsrt_last_error(ctx.handle))
        assert (out == 3.0).all() and (grad == 3.0).all() and (gdepth == 3.0).all(), over
    for k, v in arr.items():
        assert np.array_equal(v, dict(A, **kw)[k], equal_nan=True)


def test_autograd(ctx):
    """rgba.grad and depth.grad are the C call's two gradients times the upstream scalar; a colour-only loss: no depth"""
    import torch

    from gsrt.autograd import frame_loss

    W, H = 70, 37
    A, kw = inputs(W, H, 3, "all")
    want, gwant, dwant = call(ctx, W, H, 3, "all")
    dev = lambda v: torch.from_numpy(np.array(v)).to("cuda:0")  # noqa: E731
    x, d = dev(A["rgba"]).requires_grad_(True), dev(kw["depth"]).requires_grad_(True)
    y, m, t = dev(A["target"]), dev(kw["mask"]), dev(kw["target_depth"])
    loss = frame_loss(ctx, x, y, d, t, mask=m, background=BG, depth_weight=DEPTH_WEIGHT)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert np.float32(loss.item()).view(np.uint32) == np.float32(want["loss"]).view(np.uint32)
    (loss * 2.5).backward()
    assert np.array_equal(bits(x.grad.cpu().numpy()), bits(np.float32(2.5) * gwant))
    assert np.array_equal(bits(d.grad.cpu().numpy()), bits(np.float32(2.5) * dwant))
    x.grad, d.grad = None, None
    frame_loss(ctx, x, y, mask=m, background=BG).backward()
    assert d.grad is None or not d.grad.any().item()
    only, gonly, _ = gsrt.frame_loss(ctx, A["rgba"], A["target"], mask=kw["mask"], background=BG)
    assert np.array_equal(bits(x.grad.cpu().numpy()), bits(gonly))


def test_gradients_feed_the_splat_depth_gradient_frame(ctx):
    """render_depth -> frame_loss -> Scene.splat_depth_grad on a small cloud: the layouts meet (finite rows, the depth's
    slot 6 non-zero somewhere); the gradient frames have their own float64 tests"""
    W, H = 64, 48
    c, r, s, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 2000, 7, True)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        ubo = gsrt.camera_from_modelview(gsrt.lookat((0, 0, 0), (0, 0, -1)), 60.0, W, H, 1.0, 1, 16)
        rgba, depth = sc.render_depth(ubo)
        alpha = rgba[..., 3]
        seen = alpha >= np.float32(1.0 / 255.0)
        assert seen.any()
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        target = np.stack([0.5 + 0.4 * np.sin(0.3 * xx), 0.5 + 0.4 * np.cos(0.2 * yy), 0.5 + 0.0 * xx], -1).astype(np.float32)
        z = np.where(seen, depth / np.where(seen, alpha, 1.0), 0.0).astype(np.float32)
        target_depth = np.where(seen, z + 0.25, 0.0).astype(np.float32)
        mask = np.ones((H, W), np.float32)
        mask[:4] = 0.0
        out, gimg, gdepth = gsrt.frame_loss(ctx, rgba, target, mask=mask, depth=depth, target_depth=target_depth,
                                            background=(1.0, 1.0, 1.0), depth_weight=0.5)
        assert out["depth_samples"] == float(seen.sum()) and out["depth_l1"] > 0.0 and np.isfinite(out["loss"])
        assert np.isfinite(gimg).all() and np.isfinite(gdepth).all() and gdepth.any() and gimg[..., 3].any()
        rows = sc.splat_depth_grad(ubo, gimg, gdepth)
        assert rows.shape == (sc.n, 8) and np.isfinite(rows).all()
        assert rows[:, 6].any() and rows[:, :6].any()
    finally:
        sc.close()
