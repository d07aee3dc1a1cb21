"""torch.autograd glue for feature frames: learn a per-Gaussian feature table against 2-D targets.

    from gsrt.autograd import render_features
    rgba, feat = render_features(scene, ubo, table)   # table: (n, C) float32 tensor on the scene's device
    loss(feat).backward()                              # table.grad: Scene.feature_grad of the loss's gradient

and for colour frames: fit the scene's SH table (its appearance) on frozen geometry.

    from gsrt.autograd import render_colour
    rgba = render_colour(scene, ubo, sh)               # sh: (n, 16, 3) or (n, 48) float32 tensor on the scene's device
    loss(rgba).backward()                              # sh.grad: Scene.sh_grad of the loss's gradient

and for a whole model, geometry included: optimise a scene end to end.

    from gsrt.autograd import render_model
    rgba = render_model(scene, ubo, center, rot, scale, opacity, sh)
    loss(rgba).backward()                              # .grad of all five, through Scene.splat_grad and Scene.model_grad
    rgba, depth = render_model(..., depth=True)        # the expected depth too, for depth supervision

and adaptive density control between steps: render_model(..., density_stats=t) accumulates the densification statistic
in its backward, densify clones, splits and prunes the model on the device, remap_state carries optimiser state across
(the whole loop: densify's docstring).

and the loss itself: photometric_loss is 3DGS's (1 - lam) L1 + lam (1 - SSIM) of a frame against a target image in one
fused call (gsrt.image_loss), so that a training step stays in the library's kernels from the frame to the gradients:

    from gsrt.autograd import render_model, photometric_loss, image_metrics
    for step in range(steps):
        rgba = render_model(scene, ubo, center, rot, scale, opacity, sh, density_stats=stats)
        loss = photometric_loss(ctx, rgba, target, lam=0.2)   # target: (H, W, 3) or (H, W, 4) float32 GPU tensor
        loss.backward()                                       # d loss / d rgba goes straight into the gradient frames
        optimiser.step()
    image_metrics(ctx, rgba.detach(), target)                 # dict(loss=, l1=, ssim=, mse=, psnr=), no gradient

frame_loss is the same call with a background colour, a pixel mask and an L1 depth term (gsrt.frame_loss), differentiable
with respect to rgba, alpha included, and to the depth of render_model(..., depth=True) (the loop: its docstring).

and the optimiser: model_step chains the gradient tables to the raw parameters (unnormalised quaternion, log scale, logit
opacity), takes the Adam step and writes the next frame's scene arrays in one fused call (gsrt.model_step), so that a whole
training loop needs neither torch.autograd nor torch.optim (the loop: model_step's docstring).

torch is imported here only; `import gsrt` never needs it.

Synchronisation is plain and blocking: the current torch stream is synchronised before the library reads a tensor, and
Context.synchronize() returns before torch reads what the library wrote. The library's frames run on its own stream
(Context.stream), so nothing is shared with torch's stream ordering.
"""
import torch

import math

from . import MODE_COR, density_stats_add, image_loss
from . import densify as _densify
from . import frame_loss as _frame_loss
from . import frame_loss_params as _frame_loss_params
from . import model_step as _model_step


class _RenderFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, scene, ubo, mode, k):
        if table.dim() != 2 or table.shape[0] != scene.n or table.dtype != torch.float32 or not table.is_cuda:
            raise ValueError("render_features: table must be an (n, C) float32 tensor on the GPU")
        table = table.contiguous()
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        C = int(table.shape[1])
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device=table.device)
        feat = torch.empty((H, W, C), dtype=torch.float32, device=table.device)
        torch.cuda.current_stream(table.device).synchronize()
        scene.set_features(table.data_ptr(), C)  # copied into the scene's own rows
        scene.render_features_async(ubo, mode, k, rgba.data_ptr(), feat.data_ptr())
        scene.ctx.synchronize()
        ctx.scene, ctx.ubo, ctx.mode, ctx.k, ctx.shape = scene, ubo.copy(), mode, k, (scene.n, C)  # the camera as it is now
        ctx.mark_non_differentiable(rgba)
        return rgba, feat

    @staticmethod
    def backward(ctx, _grad_rgba, grad_feat):
        n, C = ctx.shape
        g = grad_feat.to(torch.float32).contiguous()
        out = torch.empty((n, C), dtype=torch.float32, device=g.device)
        torch.cuda.current_stream(g.device).synchronize()
        ctx.scene.feature_grad_async(ctx.ubo, g.data_ptr(), C, out.data_ptr(), False, ctx.mode, ctx.k)
        ctx.scene.ctx.synchronize()
        return out, None, None, None, None


def render_features(scene, ubo, table, mode=MODE_COR, k=0):
    """One feature frame of `table` ((n, C) float32 GPU tensor, 1 <= C <= gsrt.MAX_FEATURES) as torch tensors
    (rgba[H, W, 4], feat[H, W, C]), differentiable with respect to `table`: the backward is Scene.feature_grad_async of
    the upstream gradient of feat. rgba (the normaliser, r = g = b = sum w) is non-differentiable. The table is copied
    into the scene (Scene.set_features). Blocking synchronisation on both sides: torch's current stream before each
    library call, Context.synchronize() after it.
    The backward renders the scene again: it keeps a copy of `ubo`, but the scene's geometry (Scene.update, refits,
    attached arrays, streamed pages) must stay as it was in the forward until backward has run, or the gradient is that
    of another frame. The forward leaves `table` as the scene's feature table."""
    return _RenderFeatures.apply(table, scene, ubo, mode, k)


class _RenderColour(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sh, scene, ubo, mode, k):
        if sh.dtype != torch.float32 or not sh.is_cuda or tuple(sh.shape) not in ((scene.n, 16, 3), (scene.n, 48)):
            raise ValueError("render_colour: sh must be an (n, 16, 3) or (n, 48) float32 tensor on the GPU")
        table = sh.contiguous()
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device=sh.device)
        torch.cuda.current_stream(sh.device).synchronize()
        scene.set_sh(table.data_ptr())  # copied into the scene's own rows
        scene.render_async(ubo, mode, k, rgba.data_ptr())
        scene.ctx.synchronize()
        ctx.scene, ctx.ubo, ctx.mode, ctx.k, ctx.shape = scene, ubo.copy(), mode, k, tuple(sh.shape)  # the camera as it is now
        return rgba

    @staticmethod
    def backward(ctx, grad_rgba):
        g = grad_rgba.to(torch.float32).contiguous()
        out = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        torch.cuda.current_stream(g.device).synchronize()
        ctx.scene.sh_grad_async(ctx.ubo, g.data_ptr(), out.data_ptr(), False, ctx.mode, ctx.k)
        ctx.scene.ctx.synchronize()
        return out, None, None, None, None


def render_colour(scene, ubo, sh, mode=MODE_COR, k=0):
    """One colour frame of the SH table `sh` ((n, 16, 3) or (n, 48) float32 GPU tensor, [gauss][coef][rgb]) as a torch
    tensor rgba[H, W, 4], differentiable with respect to `sh`: the backward is Scene.sh_grad_async of the upstream
    gradient (alpha's share is ignored: alpha does not depend on SH). The table is copied into the scene (Scene.set_sh).
    Blocking synchronisation on both sides: torch's current stream before each library call, Context.synchronize()
    after it.
    The backward renders the scene again: it keeps a copy of `ubo`, but the scene's geometry (Scene.update, refits,
    attached arrays, streamed pages) and its SH rows must stay as they were in the forward until backward has run, or
    the gradient is that of another frame. The forward leaves `sh` as the scene's SH table."""
    return _RenderColour.apply(sh, scene, ubo, mode, k)


def _device_params(scene, device):
    """The scene's GaussParam array as an (n, 12) torch tensor on `device`, made once per scene from Scene.download and
    kept on the scene: render_rgba writes the opacities into its column 3 and hands it to Scene.update by address."""
    t = getattr(scene, "_autograd_params", None)
    if t is None or t.device != device:
        params, _ = scene.download()
        t = torch.from_numpy(params).to(device)
        scene._autograd_params = t
    return t


class _RenderRgba(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacity, sh, scene, ubo, mode, k):
        if opacity.dtype != torch.float32 or not opacity.is_cuda or tuple(opacity.shape) != (scene.n,):
            raise ValueError("render_rgba: opacity must be an (n,) float32 tensor on the GPU")
        if sh is not None and (sh.dtype != torch.float32 or not sh.is_cuda or
                               tuple(sh.shape) not in ((scene.n, 16, 3), (scene.n, 48))):
            raise ValueError("render_rgba: sh must be an (n, 16, 3) or (n, 48) float32 tensor on the GPU")
        params = _device_params(scene, opacity.device)
        params[:, 3] = opacity.detach()
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device=opacity.device)
        table = None if sh is None else sh.contiguous()
        torch.cuda.current_stream(opacity.device).synchronize()
        if table is not None:
            scene.set_sh(table.data_ptr())  # copied into the scene's own rows
        scene.update(params=params.data_ptr())  # copied; the AABBs do not depend on opacity, so nothing is refitted
        scene.render_async(ubo, mode, k, rgba.data_ptr())
        scene.ctx.synchronize()
        ctx.scene, ctx.ubo, ctx.mode, ctx.k = scene, ubo.copy(), mode, k  # the camera as it is now
        ctx.sh_shape = None if sh is None else tuple(sh.shape)
        return rgba

    @staticmethod
    def backward(ctx, grad_rgba):
        g = grad_rgba.to(torch.float32).contiguous()
        d_op = torch.empty((ctx.scene.n,), dtype=torch.float32, device=g.device)
        d_sh = None
        if ctx.sh_shape is not None and ctx.needs_input_grad[1]:
            d_sh = torch.empty(ctx.sh_shape, dtype=torch.float32, device=g.device)
        torch.cuda.current_stream(g.device).synchronize()
        ctx.scene.opacity_grad_async(ctx.ubo, g.data_ptr(), d_op.data_ptr(), False, ctx.mode, ctx.k)
        if d_sh is not None:
            ctx.scene.sh_grad_async(ctx.ubo, g.data_ptr(), d_sh.data_ptr(), False, ctx.mode, ctx.k)
        ctx.scene.ctx.synchronize()
        return d_op, d_sh, None, None, None, None


def render_rgba(scene, ubo, opacity, sh=None, mode=MODE_COR, k=0):
    """One colour frame of the opacities `opacity` ((n,) float32 GPU tensor) and, when given, the SH table `sh` ((n, 16, 3)
    or (n, 48) float32 GPU tensor, [gauss][coef][rgb]) as a torch tensor rgba[H, W, 4], differentiable with respect to
    both: the backward is Scene.opacity_grad_async of the upstream gradient, all four channels, and Scene.sh_grad_async
    of the same gradient when `sh` requires one. The forward writes `opacity` into column 3 of a device copy of the
    scene's GaussParam array (made once per scene from Scene.download and kept on the scene) and passes it to
    Scene.update; with `sh` it also calls Scene.set_sh. sh=None leaves the scene's SH rows as they are, and only the
    opacity gradient is produced. The gradient is that of gsrt.h: hits whose alpha the clamp at 0.99 cut contribute 0,
    and the set of hits, their order and the stop are not differentiated.
    Blocking synchronisation on both sides: torch's current stream before each library call, Context.synchronize()
    after it.
    The backward renders the scene again: it keeps a copy of `ubo`, but the scene's geometry (Scene.update, refits,
    attached arrays, streamed pages), its opacities and its SH rows must stay as they were in the forward until backward
    has run, or the gradient is that of another frame. The forward leaves `opacity` as the scene's opacities and `sh`
    as its SH table; a geometry change made through Scene.update by the caller is not seen by the kept copy."""
    return _RenderRgba.apply(opacity, sh, scene, ubo, mode, k)


def _add_density_stats(ctx, rows):
    """render_model(..., density_stats=t): this view's statistic from the splat rows just queued, behind them on the stream"""
    if ctx.radii is not None:  # the same statistic, with the largest screen radius beside it
        ctx.scene.view_stats_add(ctx.ubo, rows.data_ptr(), ctx.density_stats.data_ptr(), ctx.radii.data_ptr(), asynchronous=True)
    elif ctx.density_stats is not None:
        W, H = int(ctx.ubo["width"][0]), int(ctx.ubo["height"][0])
        density_stats_add(ctx.scene.ctx, rows.data_ptr(), ctx.density_stats.data_ptr(), W, H, n=ctx.scene.n,
                          asynchronous=True)


def _ubo_with_view(ubo, view):
    """render_model(..., view=V): a copy of `ubo` with V as its model_view (view[r, c] = model_view[c * 4 + r]) and V's
    inverse, computed in float64 outside the graph, as its model_view_inverse; view=None: `ubo` itself"""
    if view is None:
        return ubo
    with torch.no_grad():
        V = view.detach().to(torch.float64).cpu()
        inv = torch.linalg.inv(V)
    out = ubo.copy()
    out["model_view"][0] = V.t().contiguous().reshape(16).to(torch.float32).numpy()
    out["model_view_inverse"][0] = inv.t().contiguous().reshape(16).to(torch.float32).numpy()
    return out


def _queue_pose_grad(ctx, rows, depth):
    """render_model(..., view=V): the camera's gradient from the splat rows just queued, behind the model chain"""
    if not (ctx.has_view and ctx.needs_input_grad[5]):
        return None
    d_view = torch.empty((16,), dtype=torch.float32, device=rows.device)
    ctx.scene.pose_grad_async(ctx.ubo, rows.data_ptr(), d_view.data_ptr(), depth=depth)
    return d_view


def _view_grad(d_view):
    return None if d_view is None else d_view.reshape(4, 4).t().contiguous()  # [c][r] storage to view[r, c]


class _RenderModel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, center, cov3d, opacity, sh, aabbs, view, scene, ubo, mode, k, density_stats, radii):
        n = scene.n
        ubo = _ubo_with_view(ubo, view)
        params = torch.zeros((n, 12), dtype=torch.float32, device=center.device)  # GaussParam: centre, opacity, cov3d, pad
        params[:, 0:3], params[:, 3], params[:, 4:10] = center.detach(), opacity.detach(), cov3d.detach()
        boxes = aabbs.detach().to(torch.float32).contiguous()
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device=center.device)
        table = None if sh is None else sh.contiguous()
        torch.cuda.current_stream(center.device).synchronize()
        if table is not None:
            scene.set_sh(table.data_ptr())  # copied into the scene's own rows
        scene.update(params=params.data_ptr(), aabbs=boxes.data_ptr())  # copied
        scene.refit_bvh()  # the BVH's boxes follow the new AABBs
        scene.render_async(ubo, mode, k, rgba.data_ptr())
        scene.ctx.synchronize()
        ctx.scene, ctx.ubo, ctx.mode, ctx.k = scene, ubo.copy(), mode, k  # the camera as it is now
        ctx.sh_shape = None if sh is None else tuple(sh.shape)
        ctx.density_stats, ctx.radii = density_stats, radii
        ctx.has_view = view is not None
        return rgba

    @staticmethod
    def backward(ctx, grad_rgba):
        n = ctx.scene.n
        g = grad_rgba.to(torch.float32).contiguous()
        rows = torch.empty((n, 8), dtype=torch.float32, device=g.device)
        d_c = torch.empty((n, 3), dtype=torch.float32, device=g.device)
        d_v = torch.empty((n, 6), dtype=torch.float32, device=g.device)
        d_sh = None
        if ctx.sh_shape is not None and ctx.needs_input_grad[3]:
            d_sh = torch.empty(ctx.sh_shape, dtype=torch.float32, device=g.device)
        torch.cuda.current_stream(g.device).synchronize()
        ctx.scene.splat_grad_async(ctx.ubo, g.data_ptr(), rows.data_ptr(), False, ctx.mode, ctx.k)
        _add_density_stats(ctx, rows)
        ctx.scene.model_grad_async(ctx.ubo, rows.data_ptr(), d_c.data_ptr(), d_v.data_ptr(), False)
        d_view = _queue_pose_grad(ctx, rows, False)
        if d_sh is not None:
            ctx.scene.sh_grad_async(ctx.ubo, g.data_ptr(), d_sh.data_ptr(), False, ctx.mode, ctx.k)
        ctx.scene.ctx.synchronize()
        return d_c, d_v, rows[:, 5].contiguous(), d_sh, None, _view_grad(d_view), None, None, None, None, None, None


class _RenderModelDepth(torch.autograd.Function):
    """_RenderModel with the expected depth as a second differentiable output (render_model(..., depth=True))"""

    @staticmethod
    def forward(ctx, center, cov3d, opacity, sh, aabbs, view, scene, ubo, mode, k, density_stats, radii):
        n = scene.n
        ubo = _ubo_with_view(ubo, view)
        params = torch.zeros((n, 12), dtype=torch.float32, device=center.device)  # GaussParam: centre, opacity, cov3d, pad
        params[:, 0:3], params[:, 3], params[:, 4:10] = center.detach(), opacity.detach(), cov3d.detach()
        boxes = aabbs.detach().to(torch.float32).contiguous()
        W, H = int(ubo["width"][0]), int(ubo["height"][0])
        rgba = torch.empty((H, W, 4), dtype=torch.float32, device=center.device)
        depth = torch.empty((H, W), dtype=torch.float32, device=center.device)
        table = None if sh is None else sh.contiguous()
        torch.cuda.current_stream(center.device).synchronize()
        if table is not None:
            scene.set_sh(table.data_ptr())  # copied into the scene's own rows
        scene.update(params=params.data_ptr(), aabbs=boxes.data_ptr())  # copied
        scene.refit_bvh()  # the BVH's boxes follow the new AABBs
        scene.render_depth_async(ubo, mode, k, rgba.data_ptr(), depth.data_ptr())
        scene.ctx.synchronize()
        ctx.scene, ctx.ubo, ctx.mode, ctx.k = scene, ubo.copy(), mode, k  # the camera as it is now
        ctx.sh_shape = None if sh is None else tuple(sh.shape)
        ctx.image = (H, W, center.device)
        ctx.density_stats, ctx.radii = density_stats, radii
        ctx.has_view = view is not None
        return rgba, depth

    @staticmethod
    def backward(ctx, grad_rgba, grad_depth):
        n = ctx.scene.n
        H, W, device = ctx.image
        # an output the loss does not use has no upstream gradient: zeros
        g = (torch.zeros((H, W, 4), dtype=torch.float32, device=device) if grad_rgba is None
             else grad_rgba.to(torch.float32).contiguous())
        gd = (torch.zeros((H, W), dtype=torch.float32, device=device) if grad_depth is None
              else grad_depth.to(torch.float32).contiguous())
        rows = torch.empty((n, 8), dtype=torch.float32, device=device)
        d_c = torch.empty((n, 3), dtype=torch.float32, device=device)
        d_v = torch.empty((n, 6), dtype=torch.float32, device=device)
        d_sh = None
        if ctx.sh_shape is not None and ctx.needs_input_grad[3]:
            d_sh = torch.empty(ctx.sh_shape, dtype=torch.float32, device=device)
        torch.cuda.current_stream(device).synchronize()
        ctx.scene.splat_depth_grad_async(ctx.ubo, g.data_ptr(), gd.data_ptr(), rows.data_ptr(), False, ctx.mode, ctx.k)
        _add_density_stats(ctx, rows)
        ctx.scene.model_grad_async(ctx.ubo, rows.data_ptr(), d_c.data_ptr(), d_v.data_ptr(), False, depth=True)
        d_view = _queue_pose_grad(ctx, rows, True)
        if d_sh is not None:  # the depth does not depend on SH
            ctx.scene.sh_grad_async(ctx.ubo, g.data_ptr(), d_sh.data_ptr(), False, ctx.mode, ctx.k)
        ctx.scene.ctx.synchronize()
        return d_c, d_v, rows[:, 5].contiguous(), d_sh, None, _view_grad(d_view), None, None, None, None, None, None


def model_covariance(rot, scale):
    """cov3d (n, 6) in GaussParam's order xx, xy, xz, yy, yz, zz from rotations (r, x, y, z) and scales, with ordinary
    differentiable torch operations: Sigma = (S R)^T (S R), R the matrix gsrt_scene_from_model builds (Sphere.hpp's)."""
    r, x, y, z = rot[:, 0], rot[:, 1], rot[:, 2], rot[:, 3]
    R = torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)], -1),
                     torch.stack([2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)], -1),
                     torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], -1)], -2)
    M = scale[:, :, None] * R  # row k of R scaled by s_k
    S = torch.einsum("nki,nkj->nij", M, M)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], -1)


def render_model(scene, ubo, center, rot, scale, opacity, sh=None, mode=MODE_COR, k=0, depth=False, density_stats=None,
                 view=None, radii=None):
    """One colour frame of a whole model as a torch tensor rgba[H, W, 4], differentiable with respect to `center` (n, 3),
    `rot` (n, 4; r, x, y, z, used as given), `scale` (n, 3), `opacity` (n,) and, when given, the SH table `sh` ((n, 16, 3)
    or (n, 48)): float32 GPU tensors for a scene of n Gaussians with a built BVH. cov3d is formed here with torch
    operations (model_covariance), the AABBs as centre +- 3 max scale; the forward passes both to Scene.update, refits
    the BVH and renders. The backward is one splat gradient frame (Scene.splat_grad_async), the projection's backward
    (Scene.model_grad_async) for the centres and cov3d, slot 5 of the splat rows for the opacities, and
    Scene.sh_grad_async when `sh` requires a gradient; torch chains cov3d back to `rot` and `scale`. The gradient is that
    of gsrt.h: clamped hits contribute 0; the hits, their order, the AABB test and the stop are not differentiated. Not
    with FLAG_LUT.
    Blocking synchronisation on both sides: torch's current stream before each library call, Context.synchronize()
    after it.
    The backward renders the scene again: it keeps a copy of `ubo`, but the scene's arrays (Scene.update, refits,
    attached arrays, streamed pages) and its SH rows must stay as they were in the forward until backward has run, or
    the gradient is that of another frame. The forward leaves the model as the scene's.
    depth=True: returns (rgba, depth), depth[H, W] the expected view depth of Scene.render_depth (premultiplied, like the
    colour), both differentiable. The forward is Scene.render_depth_async; the backward is one splat-depth gradient frame
    (Scene.splat_depth_grad_async) of both upstream gradients and the depth chain (Scene.model_grad_async(depth=True)),
    the rest as above; an output the loss does not use counts as a zero upstream gradient.
    density_stats: an (n, 2) float32 GPU tensor [sum, count], or None. When given, the backward adds this view's
    densification statistic to it (gsrt.density_stats_add of the splat rows it has just computed, on the plain path and the
    depth path alike); the caller zeroes it. None changes nothing.
    radii: an (n,) float32 GPU tensor, or None; needs density_stats. When given, the backward's statistic call is
    gsrt.view_stats_add: density_stats receives the same bits, and radii[g] becomes the largest screen radius (pixels) of
    Gaussian g over the views that saw it, for densify(..., radii=, max_screen_radius=); the caller zeroes it.
    view: a (4, 4) float32 GPU tensor, the camera's model-view matrix with view[r, c] = model_view[c * 4 + r], or None. When
    given, the forward renders with a copy of `ubo` whose model_view is `view` and whose model_view_inverse is its inverse
    (computed in float64, outside the graph), and the backward adds one Scene.pose_grad_async behind the model chain and
    returns view.grad: the partial derivative with model_view_inverse held fixed (gsrt.h, gsrt_pose_grad: everything that
    flows through the projection; the rays' share, the SH basis under a rotation, is not provided), on the plain path and
    the depth path alike. For a pose on the manifold use gsrt.pose_twist and gsrt.ubo_apply_twist. None changes nothing."""
    n = scene.n
    for name, t, shape in (("center", center, (n, 3)), ("rot", rot, (n, 4)), ("scale", scale, (n, 3)),
                           ("opacity", opacity, (n,))):
        if t.dtype != torch.float32 or not t.is_cuda or tuple(t.shape) != shape:
            raise ValueError(f"render_model: {name} must be a {shape} float32 tensor on the GPU")
    if sh is not None and (sh.dtype != torch.float32 or not sh.is_cuda or tuple(sh.shape) not in ((n, 16, 3), (n, 48))):
        raise ValueError("render_model: sh must be an (n, 16, 3) or (n, 48) float32 tensor on the GPU")
    cov3d = model_covariance(rot, scale)
    with torch.no_grad():
        rad = 3.0 * scale.max(dim=1, keepdim=True).values
        aabbs = torch.cat([center - rad, center + rad], 1)
    if density_stats is not None and (density_stats.dtype != torch.float32 or not density_stats.is_cuda or
                                      tuple(density_stats.shape) != (n, 2) or not density_stats.is_contiguous()):
        raise ValueError("render_model: density_stats must be a contiguous (n, 2) float32 tensor on the GPU")
    if view is not None and (view.dtype != torch.float32 or not view.is_cuda or tuple(view.shape) != (4, 4)):
        raise ValueError("render_model: view must be a (4, 4) float32 tensor on the GPU")
    if radii is not None and (density_stats is None or radii.dtype != torch.float32 or not radii.is_cuda or
                              tuple(radii.shape) != (n,) or not radii.is_contiguous()):
        raise ValueError("render_model: radii must be a contiguous (n,) float32 tensor on the GPU, beside density_stats")
    fn = _RenderModelDepth if depth else _RenderModel
    return fn.apply(center, cov3d, opacity, sh, aabbs, view, scene, ubo, mode, k, density_stats, radii)


def densify(ctx, center, rot, scale, opacity, sh, stats, noise, params, features=None, radii=None, max_screen_radius=0.0):
    """Adaptive density control of a model on the device (gsrt.densify, gsrt_densify_async): clone, split, prune or keep
    every Gaussian by the rule of gsrt.h and return the new model (center', rot', scale', opacity', sh', features',
    origin) as torch tensors of n_out rows, in input order; sh' / features' are None when sh / features are. ctx: the
    gsrt.Context; center (n, 3), rot (n, 4), scale (n, 3), opacity (n,), sh (n, 16, 3) / (n, 48) or None, features
    (n, C) or None, stats (n, 2) (render_model's density_stats), noise (n, 2, 3) (e.g. torch.randn: the library has no
    random numbers): float32 GPU tensors; params: gsrt.densify_params(...). The outputs are allocated at 2 n rows, which
    always suffices, and returned as trimmed views. origin (int32) holds g for Gaussian g itself and -1 - g for a row
    newly made from g: remap_state carries optimiser state across. Gradients do not flow through this call.
    radii (n,) (render_model's radii) with max_screen_radius > 0: 3DGS's screen-size prune (gsrt_densify_screen_async), a
    Gaussian whose largest screen radius is above max_screen_radius is pruned; the caller zeroes radii afterwards.

    The whole loop, with Adam moments m and v per parameter tensor:

        stats = torch.zeros((n, 2), device="cuda")
        for step in range(steps):
            rgba = render_model(scene, ubo, center, rot, scale, opacity, sh, density_stats=stats)   # 1: render,
            loss(rgba).backward()                                                                   #    backward
            optimiser.step()
            if step % k == k - 1:
                with torch.no_grad():
                    new = densify(ctx, center, rot, scale, opacity, sh, stats, torch.randn(n, 2, 3, device="cuda"),
                                  gsrt.densify_params(0.0002, split_scale, 0.005))                  # 2: densify
                    origin = new[-1]
                    m, v = remap_state(m, origin), remap_state(v, origin)                           # 3: optimiser state
                    center, rot, scale, opacity, sh = (t.clone().requires_grad_() for t in new[:5])
                    n = center.shape[0]
                    scene.close()
                    scene = gsrt.Scene.from_model_device(ctx, n, center.data_ptr(), rot.data_ptr(), scale.data_ptr(),
                                                         opacity.data_ptr(), sh.data_ptr())         # 4: the new scene
                    scene.build_bvh()
                    stats = torch.zeros((n, 2), device="cuda")                                      # 5: zero the stats
    """
    n = int(center.shape[0])
    dev = center.device
    tensors = [("center", center, (n, 3)), ("rot", rot, (n, 4)), ("scale", scale, (n, 3)), ("opacity", opacity, (n,)),
               ("stats", stats, (n, 2)), ("noise", noise, (n, 2, 3))]
    if sh is not None:
        if tuple(sh.shape) not in ((n, 16, 3), (n, 48)):
            raise ValueError("densify: sh must be an (n, 16, 3) or (n, 48) tensor")
        tensors.append(("sh", sh, tuple(sh.shape)))
    fc = 0
    if features is not None:
        fc = int(features.shape[1]) if features.dim() == 2 else -1
        tensors.append(("features", features, (n, fc)))
    if radii is not None:
        tensors.append(("radii", radii, (n,)))
    for name, t, shape in tensors:
        if t.dtype != torch.float32 or not t.is_cuda or tuple(t.shape) != shape:
            raise ValueError(f"densify: {name} must be a {shape} float32 tensor on the GPU")
    src = {name: t.detach().contiguous() for name, t, _ in tensors}
    cap = 2 * n
    new = lambda *shape: torch.empty((cap,) + shape, dtype=torch.float32, device=dev)  # noqa: E731
    out = [new(3), new(4), new(3), new(), None if sh is None else new(*sh.shape[1:]),
           None if features is None else new(fc)]
    origin = torch.empty((cap,), dtype=torch.int32, device=dev)
    n_out = torch.zeros((1,), dtype=torch.int32, device=dev)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    torch.cuda.current_stream(dev).synchronize()
    _densify(ctx, ptr(src["center"]), ptr(src["rot"]), ptr(src["scale"]), ptr(src["opacity"]), ptr(src.get("sh")),
             ptr(src["stats"]), ptr(src["noise"]), params, ptr(src.get("features")), n=n, feature_channels=fc,
             out=[ptr(t) for t in out], origin=origin.data_ptr(), cap=cap, d_n_out=n_out.data_ptr(),
             radii=None if radii is None else ptr(src["radii"]), max_screen_radius=max_screen_radius)
    ctx.synchronize()
    rows = int(n_out.item())
    return tuple(None if t is None else t[:rows] for t in out) + (origin[:rows],)


def remap_state(t, origin):
    """Rows of `t` (per-Gaussian optimiser state, e.g. an Adam moment, (n, ...)) carried across a densify: row i of the
    result is t[origin[i]] where origin[i] >= 0 (the Gaussian itself) and zeros where origin[i] < 0 (newly made: a fresh
    state)."""
    origin = origin.to(torch.int64)
    kept = origin >= 0
    out = torch.zeros((origin.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    out[kept] = t[origin[kept]]
    return out


def _check_images(name, rgba, target):
    if rgba.dtype != torch.float32 or not rgba.is_cuda or rgba.dim() != 3 or rgba.shape[2] != 4:
        raise ValueError(f"{name}: rgba must be an (H, W, 4) float32 tensor on the GPU")
    if (target.dtype != torch.float32 or target.device != rgba.device or target.dim() != 3 or
            tuple(target.shape[:2]) != tuple(rgba.shape[:2]) or target.shape[2] not in (3, 4)):
        raise ValueError(f"{name}: target must be an (H, W, 3) or (H, W, 4) float32 tensor on rgba's device")


class _PhotometricLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgba, target, gctx, lam):
        x, y = rgba.detach().contiguous(), target.detach().contiguous()
        H, W = int(x.shape[0]), int(x.shape[1])
        out = torch.empty((4,), dtype=torch.float32, device=x.device)
        grad = torch.empty((H, W, 4), dtype=torch.float32, device=x.device)
        torch.cuda.current_stream(x.device).synchronize()
        image_loss(gctx, x.data_ptr(), y.data_ptr(), lam, width=W, height=H, target_channels=int(y.shape[2]),
                   d_out=out.data_ptr(), d_grad=grad.data_ptr(), asynchronous=True)
        gctx.synchronize()
        ctx.save_for_backward(grad)
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_output):
        (kept,) = ctx.saved_tensors
        return grad_output * kept, None, None, None


def photometric_loss(ctx, rgba, target, lam=0.2):
    """3DGS's photometric loss (1 - lam) l1 + lam (1 - ssim) of a frame `rgba` ((H, W, 4) float32 GPU tensor, e.g.
    render_model's; alpha is not read) against `target` ((H, W, 3) or (H, W, 4) float32 GPU tensor), as a 0-dim tensor
    that is differentiable with respect to `rgba`. ctx: the gsrt.Context. The forward is one fused call
    (gsrt.image_loss, gsrt_image_loss_async; the formulas are in gsrt.h) that also computes d loss / d rgba and keeps it;
    the backward returns the upstream scalar times the kept gradient and nothing for `target`. The alpha slot of the
    gradient is zero. Blocking synchronisation on both sides: torch's current stream before the library call,
    Context.synchronize() after it."""
    _check_images("photometric_loss", rgba, target)
    return _PhotometricLoss.apply(rgba, target, ctx, float(lam))


class _FrameLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgba, depth, target, target_depth, mask, gctx, params):
        dev = rgba.device
        planes = [None if t is None else t.detach().contiguous() for t in (mask, depth, target_depth)]
        x, y = rgba.detach().contiguous(), target.detach().contiguous()
        H, W = int(x.shape[0]), int(x.shape[1])
        out = torch.empty((6,), dtype=torch.float32, device=dev)
        grad = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        gdepth = None if depth is None else torch.empty((H, W), dtype=torch.float32, device=dev)
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        torch.cuda.current_stream(dev).synchronize()
        _frame_loss(gctx, x.data_ptr(), y.data_ptr(), mask=ptr(planes[0]), depth=ptr(planes[1]),
                    target_depth=ptr(planes[2]), params=params, width=W, height=H, target_channels=int(y.shape[2]),
                    d_out=out.data_ptr(), d_grad=grad.data_ptr(), d_grad_depth=ptr(gdepth), asynchronous=True)
        gctx.synchronize()
        ctx.has_depth = depth is not None
        ctx.save_for_backward(*([grad] if gdepth is None else [grad, gdepth]))
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_output):
        kept = ctx.saved_tensors
        return (grad_output * kept[0], grad_output * kept[1] if ctx.has_depth else None, None, None, None, None, None)


def frame_loss(ctx, rgba, target, depth=None, target_depth=None, mask=None, background=None, lam=0.2, depth_weight=0.0,
               alpha_min=1.0 / 255.0):
    """The loss of a training frame (gsrt.frame_loss, gsrt_frame_loss_async; the formulas are in gsrt.h) as a 0-dim tensor:
    photometric_loss of `rgba` composited over `background` ((r, g, b) or None) under the pixel weights `mask` ((H, W) or
    None), plus depth_weight times the mean over all pixels of mask |depth / alpha - target_depth|, taken where
    target_depth is finite and > 0 and alpha >= alpha_min. Differentiable with respect to `rgba`, alpha included, and to
    `depth` ((H, W), premultiplied, as render_model(depth=True) returns it); target, target_depth and mask get nothing.
    All tensors float32 on rgba's device. One fused call in the forward, which keeps both gradients; the backward scales
    them by the upstream scalar. Blocking synchronisation on both sides, as photometric_loss. The depth-supervised loop:

        rgba, depth = render_model(scene, ubo, center, rot, scale, opacity, sh, depth=True)
        loss = frame_loss(ctx, rgba, target, depth, target_depth, mask=mask, background=(1, 1, 1), depth_weight=0.1)
        loss.backward()              # both gradients go into the splat-depth gradient frame as they are
        optimiser.step()"""
    _check_images("frame_loss", rgba, target)
    if (depth is None) != (target_depth is None):
        raise ValueError("frame_loss: depth and target_depth come together or not at all")
    for name, t in (("depth", depth), ("target_depth", target_depth), ("mask", mask)):
        if t is not None and (t.dtype != torch.float32 or t.device != rgba.device or
                              tuple(t.shape) != tuple(rgba.shape[:2])):
            raise ValueError(f"frame_loss: {name} must be an (H, W) float32 tensor on rgba's device")
    params = _frame_loss_params(float(lam), background, float(depth_weight), float(alpha_min))
    return _FrameLoss.apply(rgba, depth, target, target_depth, mask, ctx, params)


def image_metrics(ctx, rgba, target, lam=0.2):
    """The scalars of photometric_loss without a gradient, for evaluation: dict(loss=, l1=, ssim=, mse=, psnr=) of
    Python floats, psnr = -10 log10(mse) for images in [0, 1] (inf when mse is 0). The gradient pass is skipped."""
    _check_images("image_metrics", rgba, target)
    x, y = rgba.detach().contiguous(), target.detach().contiguous()
    torch.cuda.current_stream(x.device).synchronize()
    m = image_loss(ctx, x.data_ptr(), y.data_ptr(), lam, width=int(x.shape[1]), height=int(x.shape[0]),
                   target_channels=int(y.shape[2]))
    m["psnr"] = -10.0 * math.log10(m["mse"]) if m["mse"] > 0.0 else math.inf
    return m


def _model_tensors(name, tensors, n, dev, fc=None):
    """(center, rot, scale, opacity, sh or None, features or None) checked: contiguous float32 tensors on `dev`"""
    tensors = tuple(tensors) + (None,) * (6 - len(tensors))
    shapes = [((n, 3),), ((n, 4),), ((n, 3),), ((n,),), ((n, 48), (n, 16, 3)), None]
    for t, ok, what in zip(tensors, shapes, ("center", "rot", "scale", "opacity", "sh", "features")):
        if t is None:
            continue
        good = tuple(t.shape) in ok if ok else (t.dim() == 2 and t.shape[0] == n and (fc is None or t.shape[1] == fc))
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or not good:
            raise ValueError(f"model_step: {name}.{what} must be a contiguous float32 tensor of n rows on the model's device")
    return tensors


def model_step(ctx, raw, m, v, grads, adam, want_act=True, want_grad_raw=False, sh_degree=3):
    """One optimiser step of the raw model in the library's own kernels (gsrt.model_step, gsrt_model_step_async; the
    formulas are in gsrt.h). ctx: the gsrt.Context. raw, m, v: (center (n, 3), rot (n, 4) unnormalised, log scale (n, 3),
    logit opacity (n,), sh (n, 16, 3) / (n, 48) or None, features (n, C) or None), the two Adam moments in the same layout:
    contiguous float32 GPU tensors, all updated in place. grads: (center (n, 3), cov (n, 6), splat (n, 8), sh or None,
    features or None), the tables as Scene.model_grad_async, Scene.splat_grad_async, Scene.sh_grad_async and
    Scene.feature_grad_async write them. adam: gsrt.adam_params(..., step=t), t counting from 1.
    Returns dict(act=(center, rot, scale, opacity, sh, features) or None, params=(n, 12), aabbs=(n, 6), grad_raw=(n, 11) or
    None): the activated model (sh / features in it are raw's own tensors), the scene arrays for Scene.update, and the
    chained gradient the step used. Blocking synchronisation on both sides: torch's current stream before the call,
    Context.synchronize() after it. Gradients do not flow through this call.
    sh_degree (0..3): the active SH degree (gsrt_model_step_degree_async): the SH words above it keep their bits in raw, m
    and v; raise it as the run goes for 3DGS's ramp-up. 3 is the plain step.

    The whole loop, without torch.autograd or torch.optim (n Gaussians, a W x H target; new = torch.empty on the GPU):

        raw = [t.contiguous() for t in gsrt.model_deactivate(...)]       # or from a .ply: center, rot, log scale, logit, sh
        m, v = [torch.zeros_like(t) for t in raw], [torch.zeros_like(t) for t in raw]
        rgba, gimg, rows = new(H, W, 4), new(H, W, 4), new(n, 8)
        d_c, d_cov, d_sh, out4 = new(n, 3), new(n, 6), new(n, 48), new(4)
        for t in range(1, steps + 1):
            scene.render_async(ubo, d_rgba=rgba.data_ptr())                                     # Scene.render_async
            gsrt.image_loss(ctx, rgba.data_ptr(), target.data_ptr(), 0.2, width=W, height=H, target_channels=3,
                            d_out=out4.data_ptr(), d_grad=gimg.data_ptr(), asynchronous=True)   # image_loss
            scene.splat_grad_async(ubo, gimg.data_ptr(), rows.data_ptr())                       # splat_grad_async
            scene.model_grad_async(ubo, rows.data_ptr(), d_c.data_ptr(), d_cov.data_ptr())      # model_grad_async
            scene.sh_grad_async(ubo, gimg.data_ptr(), d_sh.data_ptr())                          # sh_grad_async
            gsrt.density_stats_add(ctx, rows.data_ptr(), stats.data_ptr(), W, H, n=n, asynchronous=True)
            out = model_step(ctx, raw, m, v, (d_c, d_cov, rows, d_sh), gsrt.adam_params(step=t, sparse=True))  # model_step
            scene.update(params=out["params"].data_ptr(), aabbs=out["aabbs"].data_ptr())        # Scene.update
            scene.refit_bvh()                                                                   #  + refit_bvh
            scene.set_sh(raw[4].data_ptr())                                                     #  + set_sh

    Every call of the loop body queues on the library's streams; only model_step waits (it returns tensors). Scene.update
    reads out["params"] / out["aabbs"] on the library's update stream: keep `out` alive until the next model_step has
    returned (or call ctx.synchronize()), so that torch does not hand their memory out again before they are read. Every few
    hundred steps: densify(ctx, *out["act"][:5], stats, noise, params) on the activated model, remap_state on every tensor
    of m and v with its origin, gsrt.model_deactivate of the new model (device addresses) for the new raw tensors, and a
    new scene from the new activated arrays (Scene.from_model_device, build_bvh), as in densify's docstring; every few
    thousand, gsrt.model_opacity_reset(ctx, raw[3].data_ptr(), m[3].data_ptr(), v[3].data_ptr(), 0.01, n=n)."""
    n, dev = int(raw[0].shape[0]), raw[0].device
    raw = _model_tensors("raw", raw, n, dev)
    fc = 0 if raw[5] is None else int(raw[5].shape[1])
    m, v = _model_tensors("m", m, n, dev, fc), _model_tensors("v", v, n, dev, fc)
    grads = tuple(grads) + (None,) * (5 - len(grads))
    for t, width, what in zip(grads, (3, 6, 8, 48, fc), ("center", "cov", "splat", "sh", "features")):
        if t is not None and (t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.numel() != n * width):
            raise ValueError(f"model_step: grads.{what} must be a contiguous float32 tensor of n x {width} on the model's device")
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    act = (new(n, 3), new(n, 4), new(n, 3), new(n), raw[4], raw[5]) if want_act else None
    params, aabbs = new(n, 12), new(n, 6)
    graw = new(n, 11) if want_grad_raw else None
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    torch.cuda.current_stream(dev).synchronize()
    _model_step(ctx, [ptr(t) for t in raw], [ptr(t) for t in m], [ptr(t) for t in v], [ptr(t) for t in grads], adam, n=n,
                feature_channels=fc, act=None if act is None else [ptr(t) for t in act], params_out=params.data_ptr(),
                aabbs_out=aabbs.data_ptr(), grad_raw=ptr(graw), asynchronous=True, sh_degree=sh_degree)
    ctx.synchronize()
    return dict(act=act, params=params, aabbs=aabbs, grad_raw=graw)
