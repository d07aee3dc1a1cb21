"""Host side of opacity gradient frames (GSRT_FLAG_OPACITY_GRAD, gsrt_render_opacity_grad): the header's declarations,
constants, NULL handles, gsrt.autograd.render_rgba and the CLI's usage errors. No device needed."""
import os
import re
import subprocess

import pytest

import gsrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "3dgs-raytrace_amd", "bin", "gsrt_render")
HEADER = open(os.path.join(ROOT, "include", "gsrt.h")).read()
ENTRY_POINTS = ["gsrt_render_opacity_grad", "gsrt_render_opacity_grad_async"]


def test_header_declares_the_flag_and_entry_points():
    m = re.search(r"GSRT_FLAG_OPACITY_GRAD\s*=\s*(0x[0-9a-fA-F]+)", HEADER)
    assert m and int(m.group(1), 16) == 0x8000
    for name in ENTRY_POINTS:
        assert re.search(r"gsrt_status\s+" + name + r"\s*\(", HEADER), name
    # opacity left the two older "Not provided" lines: only geometry stays there
    assert "geometry, opacity" not in HEADER and "geometry or opacity" not in HEADER
    assert len(re.findall(r"Not provided: gradients with respect to geometry", HEADER)) == 2


def test_constants_match_the_header():
    assert gsrt.FLAG_OPACITY_GRAD == 0x8000
    others = (gsrt.FLAG_LUT | gsrt.FLAG_STATS | gsrt.FLAG_OUT_DUMP8 | gsrt.FLAG_DEPTH | gsrt.FLAG_FEATURES |
              gsrt.FLAG_FEATURE_GRAD | gsrt.FLAG_SH_GRAD | 0xFF)
    assert not gsrt.FLAG_OPACITY_GRAD & others
    assert gsrt.lib.gsrt_abi_version() == 2  # additions only
    assert set(ENTRY_POINTS) <= set(gsrt.EXPORTS)
    for name in ("opacity_grad", "opacity_grad_async"):
        assert callable(getattr(gsrt.Scene, name))


def test_null_handles():
    assert gsrt.lib.gsrt_render_opacity_grad(None, None, gsrt.MODE_COR, 0, None, None, 0) == gsrt.E_ARG
    assert gsrt.lib.gsrt_render_opacity_grad_async(None, None, gsrt.MODE_COR, 0, None, None, 0) == gsrt.E_ARG


def test_import_gsrt_needs_no_torch():
    """torch stays out of `import gsrt`: only gsrt.autograd, which holds render_rgba, imports it"""
    src = open(os.path.join(os.path.dirname(gsrt.__file__), "__init__.py")).read()
    assert "import torch" not in src and "import autograd" not in src and "from .autograd" not in src
    auto = open(os.path.join(os.path.dirname(gsrt.__file__), "autograd.py")).read()
    assert "def render_rgba(" in auto and "def render_colour(" in auto and "def render_features(" in auto


PAIR = ["--opacity-grad", "g.bin", "--opacity-grad-out", "o.bin"]
TOGETHER = "--opacity-grad and --opacity-grad-out go together"


@pytest.mark.parametrize("argv,message", [
    (["--scene", "100", "--mode", "ref"] + PAIR, "--opacity-grad needs --mode cor"),
    (["--scene", "33"] + PAIR, "--opacity-grad needs --mode cor"),  # scene 33 defaults to REF
    (["--scene", "100", "--stats"] + PAIR, "--opacity-grad cannot be combined with --stats"),
    (["--scene", "100", "--sh", "--depth", "d.pfm"] + PAIR, "--opacity-grad cannot be combined with --depth"),
    (["--scene", "100", "--features", "f.bin", "--feature-channels", "3", "--features-out", "fo.bin"] + PAIR,
     "--opacity-grad cannot be combined with --features"),
    (["--scene", "100", "--feature-grad", "fg.bin", "--feature-channels", "3", "--feature-grad-out", "fo.bin"] + PAIR,
     "--opacity-grad cannot be combined with --feature-grad"),
    (["--scene", "100", "--sh", "--sh-grad", "sg.bin", "--sh-grad-out", "so.bin"] + PAIR,
     "--opacity-grad cannot be combined with --sh-grad"),
    (["--scene", "100", "--opacity-grad", "g.bin"], TOGETHER),
    (["--scene", "100", "--sh", "--opacity-grad-out", "o.bin"], TOGETHER),
    (["--scene", "100", "--opacity-grad"], "--opacity-grad needs a value"),
])
def test_cli_opacity_grad_usage_errors(tmp_path, argv, message):
    """Exit status 2, the parser's own message and the usage text naming the new options, decided while parsing (before
    any device is opened, so the image file need not exist), and no file written."""
    p = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2, (p.returncode, p.stderr)
    assert p.stderr.startswith("gsrt_render: " + message), p.stderr
    assert "unknown option" not in p.stderr
    assert "usage: gsrt_render" in p.stderr
    assert "[--opacity-grad FILE --opacity-grad-out FILE]" in p.stderr
    assert "gsrt_create" not in p.stderr
    assert not os.listdir(tmp_path)
