"""gsrt_model_remap: the optimiser state across a densify, bit-equal to the numpy gather (the contract of
gsrt.autograd.remap_state for a whole model in one launch).

Sizes: n_out in {0, 1, 63, 64, 65, 4097}: a partly filled wave, a full one, a second wave, and a workgroup (256 rows) with
one row in it after sixteen full ones. Origin patterns: identity, all negative, the origin of a real gsrt.densify result,
and a reversed permutation. Host arrays, device arrays, and device SH tables 4 bytes off a 16-byte boundary (the word
path of the SH copy)."""
import ctypes

import numpy as np
import pytest

import gsrt
from test_features_gpu import u32

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 4097]
WIDTHS = (3, 4, 3, 1, 48)


def state(n, with_sh, seed=5):
    rng = np.random.default_rng(seed + n)
    a = [rng.normal(0, 1, (n, w)).astype(np.float32) for w in WIDTHS]
    a[3] = a[3].reshape(n)
    if n > 4:
        a[0][1, 0], a[1][2, 3], a[3][3] = np.float32(-0.0), np.float32(np.nan), np.float32(np.inf)  # copied as bits
    return tuple(a[:4]) + ((a[4] if with_sh else None), None)


def densify_origin(ctx, n):
    """the origin of a real densify pass over n Gaussians with clones, splits, prunes and keeps"""
    rng = np.random.default_rng(17 + n)
    c, r = rng.normal(0, 1, (n, 3)).astype(np.float32), rng.normal(0, 1, (n, 4)).astype(np.float32)
    s = rng.uniform(0.01, 0.2, (n, 3)).astype(np.float32)
    o = rng.uniform(0.0, 1.0, n).astype(np.float32)
    stats = np.stack([rng.uniform(0, 2, n), np.ones(n)], 1).astype(np.float32)
    noise = rng.normal(0, 1, (n, 2, 3)).astype(np.float32)
    out = gsrt.densify(ctx, c, r, s, o, None, stats, noise, gsrt.densify_params(1.0, 0.1, 0.2))
    return out[6]


def origins(ctx, kind, n_out):
    """(origin, rows of the input)"""
    if kind == "identity":
        return np.arange(n_out, dtype=np.int32), max(n_out, 1)
    if kind == "negative":
        return (-1 - np.arange(n_out, dtype=np.int32)), 3
    if kind == "reversed":
        return np.arange(n_out, dtype=np.int32)[::-1].copy(), max(n_out, 1)
    n_in = n_out
    org = densify_origin(ctx, n_in) if n_in else np.zeros(0, np.int32)
    if n_in > 8:
        assert (org < 0).any() and (org >= 0).any()
    return org, max(n_in, 1)


def gather(arrays, org):
    out = []
    for a in arrays:
        if a is None:
            out.append(None)
            continue
        rows = u32(a)[np.maximum(org, 0)].copy()
        rows[org < 0] = 0  # +0 in every word
        out.append(rows)
    return out


@pytest.mark.parametrize("with_sh", [True, False], ids=["sh", "plain"])
@pytest.mark.parametrize("kind", ["identity", "negative", "densify", "reversed"])
@pytest.mark.parametrize("n_out", SIZES)
def test_bit_equal_to_the_numpy_gather(ctx, n_out, kind, with_sh):
    import torch

    org, n_in = origins(ctx, kind, n_out)
    src = state(n_in, with_sh)
    want = gather(src, org)
    got = gsrt.model_remap(ctx, org, src)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.shape[0] == org.size and u32(g).tobytes() == w.tobytes()
    # device arrays: aligned, and every base 4 bytes past a 16-byte boundary
    for off in (0, 1):
        def dev(a, fill=None):
            if a is None:
                return None
            t = torch.zeros(a.size + 4 + off, dtype=torch.float32, device="cuda:0")
            v = t[off:off + a.size]
            if fill is None:
                v.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
            else:
                v.fill_(fill)
            return t, v
        d_in = [dev(a) for a in src]
        d_out = [None if a is None else dev(np.zeros((org.size,) + a.shape[1:], np.float32), 9.0) for a in src]
        d_org = torch.from_numpy(org.copy()).to("cuda:0") if org.size else torch.zeros(1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ptr = lambda x: 0 if x is None else x[0].data_ptr() + 4 * off  # noqa: E731  (an empty view has no address)
        gsrt.model_remap(ctx, d_org.data_ptr(), tuple(ptr(x) for x in d_in), n_out=org.size, out=tuple(ptr(x) for x in d_out))
        for x, w in zip(d_out, want):
            if x is not None:
                assert u32(x[1].cpu().numpy()).tobytes() == w.tobytes(), (off, kind)
                tail = x[0].cpu().numpy()
                assert (tail[:off] == 0).all() and (tail[off + x[1].numel():] == 0).all()  # nothing outside the rows


def test_refusals(ctx):
    import torch

    src, org = state(8, True), np.arange(8, dtype=np.int32)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    out = [None if a is None else np.zeros_like(a) for a in src]
    s_in, s_out = gsrt.ModelArrays(*[P(a) for a in src], 0), gsrt.ModelArrays(*[P(a) for a in out], 0)

    def refused(status):
        assert status == gsrt.E_ARG and b"gsrt_model_remap" in gsrt.lib.gsrt_last_error(ctx.handle)

    L = gsrt.lib.gsrt_model_remap
    assert L(ctx.handle, 8, P(org), ctypes.byref(s_in), ctypes.byref(s_out)) == gsrt.OK
    refused(L(ctx.handle, 8, P(org), None, ctypes.byref(s_out)))
    refused(L(ctx.handle, 8, None, ctypes.byref(s_in), ctypes.byref(s_out)))                       # no origin
    refused(L(ctx.handle, 8, P(org), ctypes.byref(s_in), ctypes.byref(s_in)))                      # in place
    no_sh = gsrt.ModelArrays(*[P(a) for a in out[:4]], None, None, 0)
    refused(L(ctx.handle, 8, P(org), ctypes.byref(s_in), ctypes.byref(no_sh)))                     # sh presence disagrees
    feat = gsrt.ModelArrays(*[P(a) for a in out[:5]], None, 4)
    refused(L(ctx.handle, 8, P(org), ctypes.byref(s_in), ctypes.byref(feat)))                      # channels without features
    missing = gsrt.ModelArrays(P(out[0]), None, P(out[2]), P(out[3]), P(out[4]), None, 0)
    refused(L(ctx.handle, 8, P(org), ctypes.byref(s_in), ctypes.byref(missing)))                   # a NULL array
    refused(L(ctx.handle, 0x80000000, P(org), ctypes.byref(s_in), ctypes.byref(s_out)))            # above GSRT_MAX_GAUSSIANS
    d_rot = torch.zeros(32, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    mixed = gsrt.ModelArrays(P(out[0]), d_rot.data_ptr(), P(out[2]), P(out[3]), P(out[4]), None, 0)
    refused(L(ctx.handle, 8, P(org), ctypes.byref(s_in), ctypes.byref(mixed)))                     # host and device mixed
    refused(gsrt.lib.gsrt_model_remap_async(ctx.handle, 8, P(org), ctypes.byref(s_in), ctypes.byref(s_out)))  # host, async
    assert L(ctx.handle, 0, None, ctypes.byref(s_in), ctypes.byref(s_out)) == gsrt.OK              # nothing to do
