"""The optimiser step with an active SH degree (gsrt_model_step_degree) against gsrt.model_step itself.

n in {1, 65, 513}: one lane's worth, a second wave, and a third 256-lane workgroup of the row kernel (12 float4 lanes a
row: 513 rows are 6156 lanes, 25 workgroups, the last partly filled). Degrees 0..3: the limits 3, 12 and 27 are no
multiples of 4, so on the float4 path the lanes holding words 0..3, 12..15 and 24..27 straddle them. Bases 16-byte aligned
(W == 4) and offset by 4 bytes (W == 1), with and without GSRT_ADAM_SPARSE.

The inactive words of raw, m and v (>= 3 (d + 1)^2) are overwritten with sentinels, NaN patterns included, before the call
and must keep their bits; the active words, and every other array, equal gsrt.model_step's on the case's own arrays (Adam
is per word, so the sentinels reach no active word). act rows are written for all words. Degree 3 is gsrt.model_step
everywhere: raw, m, v, act, params_out and aabbs_out."""
import ctypes

import numpy as np
import pytest

import gsrt
import model_step_ref as R
from test_features_gpu import u32

pytestmark = pytest.mark.gpu

SENTINELS = np.array([0x7FC00123, 0xFFC00001, 0x80000000, 0x7F800000, 0x7149F2CA, 0x00000001], np.uint32)
_REF = {}


def reference(ctx, n, sparse):
    """gsrt.model_step (host form) of the case: raw', m', v' and its outputs, once per (n, sparse)"""
    if (n, sparse) not in _REF:
        k = R.case(n, with_sh=True)
        raw, m, v = k.copies()
        out = gsrt.model_step(ctx, raw, m, v, k.grads, k.adam(gsrt, sparse=sparse))
        _REF[(n, sparse)] = (raw, m, v, out)
    return _REF[(n, sparse)]


def with_sentinels(sh, limit, salt):
    out = np.ascontiguousarray(sh, np.float32).reshape(-1, 48).copy()
    w = u32(out)
    idx = (np.arange(w.shape[0])[:, None] * 7 + np.arange(48)[None, :] + salt) % len(SENTINELS)
    w[:, limit:] = SENTINELS[idx][:, limit:]
    return out


def on_device(arrays, offset):
    import torch

    out = []
    for a in arrays:
        if a is None:
            out.append(None)
            continue
        t = torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to("cuda:0")
        if offset:  # a view one float in: no base is 16-byte aligned
            t = torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].reshape(t.shape)
        out.append(t)
    return out


def step_degree(ctx, n, raw, m, v, grads, adam, degree, act, params, aabbs):
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    s = [gsrt.ModelArrays(*[ptr(t) for t in set6], 0) for set6 in (raw, m, v, act)]
    g = gsrt.ModelGrads(*[ptr(t) for t in grads])
    return gsrt.lib.gsrt_model_step_degree(ctx.handle, n, ctypes.byref(s[0]), ctypes.byref(s[1]), ctypes.byref(s[2]),
                                           ctypes.byref(g), ctypes.byref(adam), degree, ctypes.byref(s[3]),
                                           ctypes.c_void_p(params.data_ptr()), ctypes.c_void_p(aabbs.data_ptr()), None)


@pytest.mark.parametrize("sparse", [False, True], ids=["dense", "sparse"])
@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset4"])
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 65, 513])
def test_inactive_words_keep_their_bits(ctx, n, degree, offset, sparse):
    import torch

    k = R.case(n, with_sh=True)
    ref_raw, ref_m, ref_v, ref_out = reference(ctx, n, sparse)
    limit = 3 * (degree + 1) ** 2
    start = [list(t) for t in k.copies()]
    for salt, t in enumerate(start):
        t[4] = with_sentinels(t[4], limit, salt)
    raw, m, v = (on_device(t, offset) for t in start)
    grads = on_device(k.grads, offset)
    act = on_device([np.zeros_like(a) for a in start[0][:4]] + [np.full((n, 48), 7.0, np.float32), None], offset)
    params, aabbs = on_device([np.zeros((n, 12), np.float32), np.zeros((n, 6), np.float32)], False)
    assert (raw[4].data_ptr() % 16 == 4) == offset
    torch.cuda.synchronize()
    adam = k.adam(gsrt, sparse=sparse)
    assert step_degree(ctx, n, raw, m, v, grads, adam, degree, act, params, aabbs) == gsrt.OK, \
        gsrt.lib.gsrt_last_error(ctx.handle).decode()
    moved = False
    for which, got, want, before in (("raw", raw, ref_raw, start[0]), ("m", m, ref_m, start[1]), ("v", v, ref_v, start[2])):
        for f, name in enumerate(("center", "rot", "scale", "opacity")):
            assert u32(got[f].cpu().numpy()).tobytes() == u32(want[f]).tobytes(), (which, name)
        g, w, b = u32(got[4].cpu().numpy()).reshape(n, 48), u32(want[4]).reshape(n, 48), u32(before[4]).reshape(n, 48)
        assert np.array_equal(g[:, limit:], b[:, limit:]), (which, "inactive words")
        assert np.array_equal(g[:, :limit], w[:, :limit]), (which, "active words")
        moved = moved or not np.array_equal(g[:, :limit], b[:, :limit])
    assert moved == bool(not sparse or k.seen.any())  # (the one Gaussian of n = 1 is not seen)
    # act, params, aabbs: written for all words, from the updated raw values
    assert np.array_equal(u32(act[4].cpu().numpy()).reshape(n, 48), u32(raw[4].cpu().numpy()).reshape(n, 48))
    for f in range(4):
        assert u32(act[f].cpu().numpy()).tobytes() == u32(ref_out["act"][f]).tobytes()
    assert params.cpu().numpy().tobytes() == ref_out["params"].tobytes()
    assert aabbs.cpu().numpy().tobytes() == ref_out["aabbs"].tobytes()
    if degree == 3:  # gsrt.model_step everywhere
        assert u32(raw[4].cpu().numpy()).tobytes() == u32(ref_raw[4]).tobytes()
        assert u32(act[4].cpu().numpy()).tobytes() == u32(ref_out["act"][4]).tobytes()


def test_python_keyword_and_host_form(ctx):
    """gsrt.model_step(sh_degree=) on host arrays and gsrt.autograd.model_step(sh_degree=) on tensors: the same bits"""
    import torch

    from gsrt.autograd import model_step

    n, degree, limit = 65, 1, 12
    k = R.case(n, with_sh=True)
    ref_raw, ref_m, ref_v, _ = reference(ctx, n, True)
    raw, m, v = k.copies()
    gsrt.model_step(ctx, raw, m, v, k.grads, k.adam(gsrt, sparse=True), sh_degree=degree)
    d_raw, d_m, d_v = (on_device(t, False) for t in k.copies())
    model_step(ctx, d_raw, d_m, d_v, on_device(k.grads, False), k.adam(gsrt, sparse=True), sh_degree=degree)
    torch.cuda.synchronize()
    for got, dev, want, before in ((raw, d_raw, ref_raw, k.raw), (m, d_m, ref_m, k.m), (v, d_v, ref_v, k.v)):
        g, w, b = (u32(a).reshape(n, 48) for a in (got[4], want[4], before[4]))
        assert np.array_equal(g[:, :limit], w[:, :limit]) and np.array_equal(g[:, limit:], b[:, limit:])
        assert not np.array_equal(w[:, limit:], b[:, limit:])  # the full step moves them
        for f in range(5):
            assert u32(dev[f].cpu().numpy()).tobytes() == u32(got[f]).tobytes()


def test_refusals_and_no_sh(ctx):
    k = R.case(65, with_sh=True)
    raw, m, v = k.copies()
    with pytest.raises(gsrt.GsrtError) as e:
        gsrt.model_step(ctx, raw, m, v, k.grads, k.adam(gsrt), sh_degree=4)
    assert e.value.status == gsrt.E_ARG and "sh_degree" in str(e.value)
    assert all(u32(a).tobytes() == u32(b).tobytes() for a, b in zip(raw[:5], k.raw[:5]))
    # a model without SH ignores the degree
    p = R.case(65, with_sh=False)
    want, got = p.copies(), p.copies()
    gsrt.model_step(ctx, *want, p.grads, p.adam(gsrt))
    gsrt.model_step(ctx, *got, p.grads, p.adam(gsrt), sh_degree=0)
    for a3, b3 in zip(want, got):
        assert all(u32(a).tobytes() == u32(b).tobytes() for a, b in zip(a3[:4], b3[:4]))
