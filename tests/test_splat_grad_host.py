"""Host side of splat gradient frames (GSRT_FLAG_SPLAT_GRAD, gsrt_render_splat_grad, gsrt_splat_grad_to_model): the header's
declarations, constants, NULL handles, gsrt.autograd.render_model and the CLI's usage errors. No device needed."""
import os
import re
import subprocess

import pytest

import gsrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "3dgs-raytrace_amd", "bin", "gsrt_render")
HEADER = open(os.path.join(ROOT, "include", "gsrt.h")).read()
ENTRY_POINTS = ["gsrt_render_splat_grad", "gsrt_render_splat_grad_async", "gsrt_splat_grad_to_model",
                "gsrt_splat_grad_to_model_async"]


def test_header_and_constants():
    m = re.search(r"GSRT_FLAG_SPLAT_GRAD\s*=\s*(0x[0-9a-fA-F]+)", HEADER)
    assert m and int(m.group(1), 16) == 0x20000 == gsrt.FLAG_SPLAT_GRAD
    for name in ENTRY_POINTS:
        assert re.search(r"gsrt_status\s+" + name + r"\s*\(", HEADER), name
    others = (gsrt.FLAG_LUT | gsrt.FLAG_STATS | gsrt.FLAG_OUT_DUMP8 | gsrt.FLAG_DEPTH | gsrt.FLAG_FEATURES |
              gsrt.FLAG_FEATURE_GRAD | gsrt.FLAG_SH_GRAD | gsrt.FLAG_OPACITY_GRAD | 0x10000 | 0xFF)
    assert not gsrt.FLAG_SPLAT_GRAD & others
    assert gsrt.lib.gsrt_abi_version() == 2  # additions only
    assert set(ENTRY_POINTS) <= set(gsrt.EXPORTS)
    for name in ("splat_grad", "splat_grad_async", "model_grad", "model_grad_async", "geometry_grad"):
        assert callable(getattr(gsrt.Scene, name))
    auto = open(os.path.join(os.path.dirname(gsrt.__file__), "autograd.py")).read()
    assert "def render_model(" in auto


def test_null_handles():
    L = gsrt.lib
    assert L.gsrt_render_splat_grad(None, None, gsrt.MODE_COR, 0, None, None, 0) == gsrt.E_ARG
    assert L.gsrt_render_splat_grad_async(None, None, gsrt.MODE_COR, 0, None, None, 0) == gsrt.E_ARG
    assert L.gsrt_splat_grad_to_model(None, None, None, None, None, 0) == gsrt.E_ARG
    assert L.gsrt_splat_grad_to_model_async(None, None, None, None, None, 0) == gsrt.E_ARG


PAIR = ["--splat-grad", "g.bin", "--splat-grad-out", "o.bin"]
TOGETHER = "--splat-grad and --splat-grad-out go together"


@pytest.mark.parametrize("argv,message", [
    (["--scene", "100", "--mode", "ref"] + PAIR, "--splat-grad needs --mode cor"),
    (["--scene", "33"] + PAIR, "--splat-grad needs --mode cor"),  # scene 33 defaults to REF
    (["--scene", "100", "--stats"] + PAIR, "--splat-grad cannot be combined with --stats"),
    (["--scene", "100", "--sh", "--depth", "d.pfm"] + PAIR, "--splat-grad cannot be combined with --depth"),
    (["--scene", "100", "--opacity-grad", "og.bin", "--opacity-grad-out", "oo.bin"] + PAIR,
     "--splat-grad cannot be combined with --opacity-grad"),
    (["--scene", "100", "--sh", "--sh-grad", "sg.bin", "--sh-grad-out", "so.bin"] + PAIR,
     "--splat-grad cannot be combined with --sh-grad"),
    (["--scene", "100", "--splat-grad", "g.bin"], TOGETHER),
    (["--scene", "100", "--splat-grad-out", "o.bin"], TOGETHER),
    (["--scene", "100", "--splat-grad"], "--splat-grad needs a value"),
])
def test_cli_splat_grad_usage_errors(tmp_path, argv, message):
    """Exit status 2, the parser's own message and the usage text naming the new options, decided while parsing (before
    any device is opened), and no file written."""
    p = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2, (p.returncode, p.stderr)
    assert p.stderr.startswith("gsrt_render: " + message), p.stderr
    assert "unknown option" not in p.stderr
    assert "[--splat-grad FILE --splat-grad-out FILE]" in p.stderr
    assert "gsrt_create" not in p.stderr
    assert not os.listdir(tmp_path)
