"""Host side of feature frames (GSRT_FLAG_FEATURES): constants, NULL handles and the CLI's usage errors. No device
needed."""
import os
import subprocess

import pytest

import gsrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "3dgs-raytrace_amd", "bin", "gsrt_render")


def test_flag_value_and_abi():
    assert gsrt.FLAG_FEATURES == 0x1000 and gsrt.MAX_FEATURES == 16
    others = gsrt.FLAG_LUT | gsrt.FLAG_STATS | gsrt.FLAG_OUT_DUMP8 | gsrt.FLAG_DEPTH | 0xFF
    assert not gsrt.FLAG_FEATURES & others
    assert gsrt.lib.gsrt_abi_version() == 2  # additions only


def test_null_handles():
    assert gsrt.lib.gsrt_feature_buffer(None) is None
    assert gsrt.lib.gsrt_scene_features(None) == 0
    assert gsrt.lib.gsrt_scene_set_features(None, None, 0) == gsrt.E_ARG


PAIR = ["--features", "f.bin", "--feature-channels", "3", "--features-out", "o.bin"]


@pytest.mark.parametrize("argv", [
    ["--scene", "100", "--mode", "ref"] + PAIR,
    ["--scene", "33"] + PAIR,  # scene 33 defaults to REF
    ["--scene", "100", "--stats"] + PAIR,
    ["--scene", "100", "--depth", "d.pfm"] + PAIR,
    ["--scene", "100", "--features", "f.bin", "--feature-channels", "0", "--features-out", "o.bin"],
    ["--scene", "100", "--features", "f.bin", "--feature-channels", "17", "--features-out", "o.bin"],
    ["--scene", "100", "--features", "f.bin", "--feature-channels", "3"],  # no --features-out
    ["--scene", "100", "--features-out", "o.bin"],  # no table
    ["--scene", "100", "--features", "f.bin", "--features-out", "o.bin"],  # no channel count
    ["--scene", "100", "--feature-channels", "3"],
    ["--scene", "100", "--features"],
])
def test_cli_features_usage_errors(tmp_path, argv):
    """The feature options with --mode ref (or a scene whose default mode is REF), --stats or --depth, a channel count
    outside 1..16, or one option without the others: exit status 2 and the usage text, decided while parsing (before
    any device is opened, so the table file need not exist), and no file written."""
    p = subprocess.run([CLI] + argv, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2, (p.returncode, p.stderr)
    assert "usage: gsrt_render" in p.stderr and "--features" in p.stderr
    assert "gsrt_create" not in p.stderr
    assert not os.listdir(tmp_path)
