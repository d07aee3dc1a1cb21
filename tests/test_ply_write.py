"""gsrt_ply_write: the raw model as a binary little-endian 3DGS .ply. A numpy parser here reads the header and the body
back; gsrt_ply_info / gsrt_ply_read read the same file. No device."""
import ctypes
import os

import numpy as np
import pytest

import gsrt

PROPS_SH = (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(45)] +
            ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])
PROPS_PLAIN = [p for p in PROPS_SH if not p.startswith("f_")]


def raw_model(n, with_sh, seed=11):
    rng = np.random.default_rng(seed)
    c = rng.normal(0, 2, (n, 3)).astype(np.float32)
    q = rng.normal(0, 1, (n, 4)).astype(np.float32)            # unnormalised
    ls = rng.uniform(-6, -2, (n, 3)).astype(np.float32)         # log scale
    lo = rng.normal(0, 3, n).astype(np.float32)                 # logit
    sh = rng.normal(0, 0.5, (n, 16, 3)).astype(np.float32) if with_sh else None
    if n > 2:
        c[1, 0], lo[2] = np.float32(-0.0), np.float32(np.inf)   # written as the bits they are
    return c, q, ls, lo, sh


def parse(path):
    """header property list and the body as a float32 (n, properties) array"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode().splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and lines[-1] == "end_header"
    n = int(lines[2].split()[2])
    assert lines[2] == f"element vertex {n}"
    props = []
    for ln in lines[3:-1]:
        kind, typ, name = ln.split()
        assert kind == "property" and typ == "float"
        props.append(name)
    body = np.frombuffer(data[end:], "<f4")
    assert body.size == n * len(props)
    return props, body.reshape(n, len(props))


@pytest.mark.parametrize("with_sh", [True, False], ids=["sh", "plain"])
@pytest.mark.parametrize("n", [0, 1, 37])
def test_write_and_read_back(tmp_path, n, with_sh):
    c, q, ls, lo, sh = raw_model(n, with_sh)
    path = tmp_path / "model.ply"
    gsrt.ply_write(path, c, q, ls, lo, sh)
    props, body = parse(path)
    assert props == (PROPS_SH if with_sh else PROPS_PLAIN)
    col = {name: body[:, i] for i, name in enumerate(props)}
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    for k, name in enumerate("xyz"):
        assert (bits(col[name]) == bits(c[:, k])).all()
        assert not bits(col["n" + name]).any()                              # normals: +0
        assert (bits(col[f"scale_{k}"]) == bits(ls[:, k])).all()
    for k in range(4):
        assert (bits(col[f"rot_{k}"]) == bits(q[:, k])).all()
    assert (bits(col["opacity"]) == bits(lo)).all()
    if with_sh:
        for ch in range(3):
            assert (bits(col[f"f_dc_{ch}"]) == bits(sh[:, 0, ch])).all()
            for j in range(15):                                             # channel-major
                assert (bits(col[f"f_rest_{ch * 15 + j}"]) == bits(sh[:, 1 + j, ch])).all()
    # the library's own reader
    assert gsrt.ply_info(path) == {"n": n, "sh_degree": 3 if with_sh else 0}
    gc, gq, gs, go, gsh = gsrt.ply_read(path)
    assert bits(gc).tobytes() == bits(c).tobytes()
    if with_sh:
        assert bits(gsh).tobytes() == bits(sh.reshape(n, 48)).tobytes()     # the SH table bit for bit
    else:
        assert not gsh.any()
    # the reader's activations, held as tests/test_ply.py holds them
    wq = q / np.sqrt((q * q).sum(1, keepdims=True))
    finite = np.isfinite(lo)
    np.testing.assert_allclose(gq, wq, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(gs, np.exp(ls), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(go[finite], 1.0 / (1.0 + np.exp(-lo[finite])), rtol=2e-6, atol=1e-7)
    if n > 2:
        assert go[2] == 1.0                                                 # logit +inf


def test_refusals(tmp_path):
    c, q, ls, lo, sh = raw_model(5, True)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    good = gsrt.ModelArrays(P(c), P(q), P(ls), P(lo), P(sh), None, 0)
    path = os.fsencode(tmp_path / "x.ply")
    assert gsrt.lib.gsrt_ply_write(path, 5, ctypes.byref(good)) == gsrt.OK
    assert gsrt.lib.gsrt_ply_write(None, 5, ctypes.byref(good)) == gsrt.E_ARG
    assert gsrt.lib.gsrt_ply_write(path, 5, None) == gsrt.E_ARG
    assert gsrt.lib.gsrt_ply_write(path, 5, ctypes.byref(gsrt.ModelArrays(P(c), None, P(ls), P(lo), P(sh), None, 0))) == gsrt.E_ARG
    feat = np.zeros((5, 4), np.float32)
    assert gsrt.lib.gsrt_ply_write(path, 5, ctypes.byref(gsrt.ModelArrays(P(c), P(q), P(ls), P(lo), P(sh), P(feat), 4))) == gsrt.E_ARG
    assert gsrt.lib.gsrt_ply_write(path, 5, ctypes.byref(gsrt.ModelArrays(P(c), P(q), P(ls), P(lo), P(sh), None, 4))) == gsrt.E_ARG
    with pytest.raises(gsrt.GsrtError) as e:                                # an unwritable path
        gsrt.ply_write(tmp_path / "no_such_dir" / "x.ply", c, q, ls, lo, sh)
    assert e.value.status == gsrt.E_IO
