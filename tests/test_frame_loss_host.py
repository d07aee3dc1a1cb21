"""Host side of the frame loss (gsrt_frame_loss, gsrt_frame_loss_async): the header's declarations, the export list, the
ABI version, the params struct's size and layout, the Python names, and every refusal of the call through the Python
wrapper's own argument checks, which run before the library is entered (ctx is None throughout). No device needed."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import gsrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "3dgs-raytrace_amd", "bin", "gsrt_render")
HEADER = open(os.path.join(ROOT, "include", "gsrt.h")).read()
ENTRY_POINTS = ["gsrt_frame_loss", "gsrt_frame_loss_async"]
W, H = 6, 5


def test_header_and_exports():
    for name in ENTRY_POINTS:
        assert re.search(r"gsrt_status\s+" + name + r"\s*\(", HEADER), name
        assert hasattr(gsrt.lib, name), name
    assert set(ENTRY_POINTS) <= set(gsrt.EXPORTS)
    assert re.search(r"#define GSRT_ABI_VERSION 2\b", HEADER)
    assert gsrt.lib.gsrt_abi_version() == 2  # additions only
    assert re.search(r"#define GSRT_LOSS_BACKGROUND 1u\b", HEADER) and gsrt.LOSS_BACKGROUND == 1
    assert re.search(r"#define GSRT_FRAME_LOSS_SCALARS 6\b", HEADER) and gsrt.FRAME_LOSS_SCALARS == 6
    assert HEADER.index("gsrt_image_loss_window(") < HEADER.index("gsrt_frame_loss(") < HEADER.index("gsrt_adam_scalars(")
    section = HEADER[HEADER.index("---- frame loss"):HEADER.index("gsrt_status gsrt_frame_loss_async")]
    for text in ("rgb_c + (1 - a) * bg_c", "x'_c = m * x_c", "a >= alpha_min", "q = D / a", "depth_l1", "depth_samples",
                 "(g_0 * bg_0 + g_1 * bg_1) + g_2 * bg_2", "(kd * m) * sign(e)", "(s * q) / a", "s / a", "sign(0) = 0",
                 "bit for bit", "Not provided"):
        assert text in section, text


def test_params_struct():
    P = gsrt.FrameLossParams
    assert ctypes.sizeof(P) == 32
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("lam", 0), ("background", 4), ("depth_weight", 16), ("alpha_min", 20), ("flags", 24), ("reserved", 28)]
    block = HEADER[HEADER.index("typedef struct gsrt_frame_loss_params"):HEADER.index("} gsrt_frame_loss_params;")]
    assert re.findall(r"^\s*(?:float|uint32_t)\s+(\w+)", block, flags=re.M) == [
        "lambda", "background", "depth_weight", "alpha_min", "flags", "reserved"]
    p = gsrt.frame_loss_params()
    assert (p.lam, tuple(p.background), p.depth_weight, p.flags, p.reserved) == (np.float32(0.2), (0, 0, 0), 0.0, 0, 0)
    assert p.alpha_min == np.float32(1.0 / 255.0)
    p = gsrt.frame_loss_params(0.5, (1, 0.5, 0.25), 0.1, 0.5)
    assert (p.lam, tuple(p.background), p.depth_weight, p.alpha_min, p.flags) == (0.5, (1, 0.5, 0.25), np.float32(0.1), 0.5, 1)


def test_python_names():
    sig = inspect.signature(gsrt.frame_loss)
    assert list(sig.parameters)[:11] == ["ctx", "rgba", "target", "mask", "depth", "target_depth", "background", "lam",
                                         "depth_weight", "alpha_min", "want_grad"]
    assert sig.parameters["mask"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["lam"].default == 0.2 and sig.parameters["depth_weight"].default == 0.0
    assert sig.parameters["alpha_min"].default == 1 / 255 and sig.parameters["want_grad"].default is True
    from gsrt import autograd

    assert list(inspect.signature(autograd.frame_loss).parameters) == [
        "ctx", "rgba", "target", "depth", "target_depth", "mask", "background", "lam", "depth_weight", "alpha_min"]
    for step in ("render_model(scene, ubo, center, rot, scale, opacity, sh, depth=True)", "frame_loss(ctx, rgba, target, depth",
                 "loss.backward()"):
        assert step in autograd.frame_loss.__doc__, step
    assert list(inspect.signature(autograd.photometric_loss).parameters) == ["ctx", "rgba", "target", "lam"]  # as it was


def test_null_handles():
    L = gsrt.lib
    for fn in (L.gsrt_frame_loss, L.gsrt_frame_loss_async):
        assert fn(None, 4, 4, None, None, 3, None, None, None, None, None, None, None) == gsrt.E_ARG


def host():
    rng = np.random.default_rng(3)
    return dict(rgba=rng.uniform(0, 1, (H, W, 4)).astype(np.float32), target=rng.uniform(0, 1, (H, W, 3)).astype(np.float32),
                mask=np.ones((H, W), np.float32), depth=np.ones((H, W), np.float32), target_depth=np.ones((H, W), np.float32))


def refused(match, rgba, target, **kw):
    with pytest.raises(gsrt.GsrtError, match=match) as e:
        gsrt.frame_loss(None, rgba, target, **kw)
    assert e.value.status == gsrt.E_ARG


def test_wrapper_refuses_bad_params():
    a = host()
    nan, inf = float("nan"), float("inf")
    for kw, match in [(dict(lam=-0.01), "lam"), (dict(lam=1.01), "lam"), (dict(lam=nan), "lam"),
                      (dict(params=gsrt.frame_loss_params(flags=2)), "unknown flag"),
                      (dict(params=gsrt.frame_loss_params(flags=3)), "unknown flag"),
                      (dict(params=gsrt.frame_loss_params(reserved=1)), "reserved"),
                      (dict(params="none"), "params"),
                      (dict(background=(nan, 0, 0)), "background"), (dict(background=(0, inf, 0)), "background"),
                      (dict(background=(0, 0, -inf)), "background"),
                      (dict(depth_weight=-1.0), "depth_weight"), (dict(depth_weight=nan), "depth_weight"),
                      (dict(alpha_min=0.0), "alpha_min"), (dict(alpha_min=-0.1), "alpha_min"),
                      (dict(alpha_min=1.01), "alpha_min"), (dict(alpha_min=nan), "alpha_min")]:
        refused(match, a["rgba"], a["target"], **kw)
    # a non-finite background is read only with the flag
    p = gsrt.frame_loss_params(background=(nan, 0, 0), flags=0)
    assert gsrt._frame_loss_refusal(p, W, H, 3, [16, 4096, 0, 0, 0], 0, (0, 0)) is None


def test_wrapper_refuses_bad_arrays():
    a = host()
    refused("depth and target_depth", a["rgba"], a["target"], depth=a["depth"])
    refused("depth and target_depth", a["rgba"], a["target"], target_depth=a["target_depth"])
    refused(r"\(H, W, 4\)", a["rgba"][..., :3], a["target"])
    refused(r"\(H, W, 4\)", a["rgba"], a["target"][..., :2])
    refused(r"\(H, W, 4\)", a["rgba"], a["target"][1:])
    refused(r"\(H, W, 4\)", None, a["target"])
    refused(r"\(H, W, 4\)", a["rgba"], None)
    refused(r"\(H, W\) arrays", a["rgba"], a["target"], mask=a["mask"][1:])
    refused(r"\(H, W\) arrays", a["rgba"], a["target"], depth=a["depth"][:, 1:], target_depth=a["target_depth"])
    # host arrays and device addresses mixed, either way
    refused("mixed", a["rgba"], 4096)
    refused("mixed", 4096, a["target"], width=W, height=H, target_channels=3)
    refused("mixed", a["rgba"], a["target"], mask=4096)
    refused("mixed", a["rgba"], a["target"], d_grad=4096)
    refused("mixed", a["rgba"], a["target"], d_out=4096)
    refused("mixed", a["rgba"], a["target"], depth=a["depth"], target_depth=a["target_depth"], d_grad_depth=4096)


def test_wrapper_refuses_bad_addresses():
    px = W * H
    step = 1 << 16  # far more than any array of the frame
    x, y, m, d, t, o, g, gd = (step * (i + 1) for i in range(8))
    dims = dict(width=W, height=H, target_channels=3)
    ok = dict(mask=m, depth=d, target_depth=t, d_out=o, d_grad=g, d_grad_depth=gd, **dims)
    why = lambda **kw: gsrt._frame_loss_refusal(  # noqa: E731
        gsrt.frame_loss_params(), kw.get("width", W), kw.get("height", H), kw.get("channels", 3),
        [kw.get("x", x), kw.get("y", y), kw.get("m", m), kw.get("d", d), kw.get("t", t)], kw.get("o", o),
        (kw.get("g", g), kw.get("gd", gd)))
    assert why() is None  # the arguments the refusals below vary
    refused("need width", x, y)
    for kw in (dict(width=0), dict(height=0), dict(width=32769), dict(height=32769)):
        refused("1..32768", x, y, **dict(ok, **kw))
    for c in (0, 2, 5):
        refused("target_channels", x, y, **dict(ok, target_channels=c))
    refused("NULL", 0, y, **ok)
    refused("NULL", x, 0, **ok)
    refused("depth and target_depth", x, y, **dict(ok, depth=0))
    refused("depth and target_depth", x, y, **dict(ok, target_depth=None))
    refused("grad_depth needs", x, y, **dict(ok, depth=0, target_depth=0))
    refused("grad_depth needs", x, y, **dict(ok, d_grad=0))
    # an output on an input, on the last word of one, and on another output
    for kw in (dict(d_grad=x), dict(d_grad=y), dict(d_grad=m), dict(d_grad=d), dict(d_grad=t),
               dict(d_grad_depth=x), dict(d_grad_depth=y), dict(d_grad_depth=m), dict(d_grad_depth=d),
               dict(d_grad_depth=t), dict(d_out=x), dict(d_out=t), dict(d_out=m + 4 * px - 4),
               dict(d_grad=x + 16 * (px - 1)), dict(d_grad_depth=g + 16 * px - 4), dict(d_grad_depth=g),
               dict(d_out=g), dict(d_out=gd + 4 * (px - 1)), dict(d_grad=o - 16 * px + 16)):
        refused("overlaps", x, y, **dict(ok, **kw))
    assert why(gd=g + 16 * px) is None and why(o=gd + 4 * px) is None  # adjacent is apart
    # 16-byte alignment of rgba, grad_image and a 4-channel target on the device
    refused("16-byte", x + 4, y, **ok)
    refused("16-byte", x, y, **dict(ok, d_grad=g + 8))
    refused("16-byte", x, y + 4, **dict(ok, target_channels=4))
    assert why(y=y + 4) is None


def test_readme_and_cli_help():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"^- \*\*Frame loss", readme, flags=re.M)
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    text = out.stdout + out.stderr
    for opt in ("--loss-mask", "--loss-background", "--loss-depth-target", "--loss-depth-weight", "--loss-depth-grad-out"):
        assert opt in text, opt
    # usage errors, found while parsing: exit status 2 and the reason on stderr
    for args, why in [("--loss-mask m.bin", "go with --loss-target"),
                      ("--loss-target t.bin --loss-background 1,2", "takes r,g,b"),
                      ("--loss-target t.bin --mode cor --loss-depth-target z.bin", "needs --depth"),
                      ("--loss-target t.bin --loss-depth-weight 2", "go with --loss-depth-target"),
                      ("--loss-target t.bin --mode cor --depth d.pfm --loss-depth-target z.bin --loss-depth-grad-out g.bin",
                       "needs --loss-grad-out")]:
        out = subprocess.run([CLI] + args.split(), capture_output=True, text=True)
        assert out.returncode == 2 and why in out.stderr, (args, out.stderr[:200])
