"""torch.autograd glue for feature frames: learn a per-Gaussian feature table against 2-D targets.

    from gsrt.autograd import render_features
    rgba, feat = render_features(scene, ubo, table)   # table: (n, C) float32 tensor on the scene's device
    loss(feat).backward()                              # table.grad: Scene.feature_grad of the loss's gradient

torch is imported here only; `import gsrt` never needs it.

Synchronisation is plain and blocking: the current torch stream is synchronised before the library reads a tensor, and
Context.synchronize() returns before torch reads what the library wrote. The library's frames run on its own stream
(Context.stream), so nothing is shared with torch's stream ordering.
"""
import torch

from . import MODE_COR


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
