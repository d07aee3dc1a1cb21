"""Host side of gradient frames (GSRT_FLAG_FEATURE_GRAD, gsrt_render_feature_grad): constants, NULL handles and the
CLI's usage errors. No device needed."""
import os
import subprocess

import pytest

import gsrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "3dgs-raytrace_amd", "bin", "gsrt_render")


def test_flag_value_and_abi():
    assert gsrt.FLAG_FEATURE_GRAD == 0x2000
    others = gsrt.FLAG_LUT | gsrt.FLAG_STATS | gsrt.FLAG_OUT_DUMP8 | gsrt.FLAG_DEPTH | gsrt.FLAG_FEATURES | 0xFF
    assert not gsrt.FLAG_FEATURE_GRAD & others
    assert gsrt.lib.gsrt_abi_version() == 2  # additions only
    assert {"gsrt_render_feature_grad", "gsrt_render_feature_grad_async"} <= set(gsrt.EXPORTS)


def test_null_handles():
    assert gsrt.lib.gsrt_render_feature_grad(None, None, gsrt.MODE_COR, 0, None, 1, None, 0) == gsrt.E_ARG
    assert gsrt.lib.gsrt_render_feature_grad_async(None, None, gsrt.MODE_COR, 0, None, 1, None, 0) == gsrt.E_ARG


def test_autograd_module_is_not_imported_by_the_package():
    """torch stays out of `import gsrt`: only gsrt.autograd imports it"""
    src = open(os.path.join(os.path.dirname(gsrt.__file__), "__init__.py")).read()
    assert "import torch" not in src and "import autograd" not in src and "from .autograd" not in src
    assert os.path.exists(os.path.join(os.path.dirname(gsrt.__file__), "autograd.py"))


TRIO = ["--feature-grad", "g.bin", "--feature-channels", "3", "--feature-grad-out", "o.bin"]


TOGETHER = "--feature-grad, --feature-channels and --feature-grad-out go together"


@pytest.mark.parametrize("argv,message", [
    (["--scene", "100", "--mode", "ref"] + TRIO, "--feature-grad needs --mode cor"),
    (["--scene", "33"] + TRIO, "--feature-grad needs --mode cor"),  # scene 33 defaults to REF
    (["--scene", "100", "--stats"] + TRIO, "--feature-grad cannot be combined with --stats"),
    (["--scene", "100", "--depth", "d.pfm"] + TRIO, "--feature-grad cannot be combined with --depth"),
    (["--scene", "100", "--features", "f.bin", "--features-out", "fo.bin"] + TRIO,
     "--feature-grad cannot be combined with --features"),
    (["--scene", "100", "--feature-grad", "g.bin", "--feature-channels", "0", "--feature-grad-out", "o.bin"],
     "--feature-channels must be 1..16"),
    (["--scene", "100", "--feature-grad", "g.bin", "--feature-channels", "17", "--feature-grad-out", "o.bin"],
     "--feature-channels must be 1..16"),
    (["--scene", "100", "--feature-grad", "g.bin", "--feature-channels", "3"], TOGETHER),  # no --feature-grad-out
    (["--scene", "100", "--feature-grad-out", "o.bin", "--feature-channels", "3"], TOGETHER),  # no gradient image
    (["--scene", "100", "--feature-grad", "g.bin", "--feature-grad-out", "o.bin"], TOGETHER),  # no channel count
    (["--scene", "100", "--feature-grad-out", "o.bin"], TOGETHER),
    (["--scene", "100", "--feature-grad"], "--feature-grad needs a value"),
])
def test_cli_feature_grad_usage_errors(tmp_path, argv, message):
    """The gradient options with --mode ref (or a scene whose default mode is REF), --stats, --depth or --features, a
    channel count outside 1..16, or one option without the others: exit status 2, the parser's own message for that
    case and the usage text with the new options' line, decided while parsing (before any device is opened, so the
    image file need not exist), and no file written."""
    p = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2, (p.returncode, p.stderr)
    assert p.stderr.startswith("gsrt_render: " + message), p.stderr
    assert "unknown option" not in p.stderr
    assert "usage: gsrt_render" in p.stderr
    assert "[--feature-grad FILE --feature-channels C --feature-grad-out FILE]" in p.stderr
    assert "gsrt_create" not in p.stderr
    assert not os.listdir(tmp_path)
