"""The training session without a device: every gsrt_trainer entry point refuses a NULL handle, and the gsrt_train CLI
refuses bad command lines with a usage line."""
import ctypes
import os
import subprocess

import pytest

import gsrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(ROOT, "3dgs-raytrace_amd", "bin", "gsrt_train")


def test_null_handles_are_refused():
    L = gsrt.lib
    h = ctypes.c_void_p()
    u = ctypes.c_uint32(7)
    model = gsrt.ModelArrays()
    assert L.gsrt_trainer_create(None, ctypes.byref(model), 1, 1, ctypes.byref(h)) == gsrt.E_ARG and not h.value
    L.gsrt_trainer_destroy(None)  # a no-op
    adam, loss, dens = gsrt.adam_params(), gsrt.frame_loss_params(), gsrt.densify_params(1.0, 1.0, 0.0)
    assert L.gsrt_trainer_step(None, None, 0, None, 3, None, None, ctypes.byref(loss), ctypes.byref(adam), None) == gsrt.E_ARG
    assert L.gsrt_trainer_densify(None, ctypes.byref(dens), 0, ctypes.byref(u)) == gsrt.E_ARG and u.value == 7
    assert L.gsrt_trainer_opacity_reset(None, 0.01) == gsrt.E_ARG
    assert L.gsrt_trainer_rebuild_bvh(None) == gsrt.E_ARG
    assert L.gsrt_trainer_scene(None, ctypes.byref(h)) == gsrt.E_ARG and not h.value
    assert L.gsrt_trainer_info(None, ctypes.byref(u), None, None) == gsrt.E_ARG and u.value == 7
    assert L.gsrt_trainer_state(None, ctypes.byref(model), None, None, None, None) == gsrt.E_ARG
    assert L.gsrt_trainer_download(None, ctypes.byref(model), None) == gsrt.E_ARG
    # the two device calls the trainer is built on
    assert L.gsrt_normal_noise(None, 4, 0, 0, None) == gsrt.E_ARG
    assert L.gsrt_model_remap(None, 0, None, ctypes.byref(model), ctypes.byref(model)) == gsrt.E_ARG


@pytest.mark.parametrize("args", [
    [],
    ["--ply", "a.ply"],
    ["--ply", "a.ply", "--views", "v.txt", "--out", "o.ply", "--width", "0", "--height", "8", "--fovy", "60", "--iters", "1"],
    ["--ply", "a.ply", "--views", "v.txt", "--out", "o.ply", "--width", "8", "--height", "8", "--fovy", "60", "--iters", "x"],
    ["--ply", "a.ply", "--views", "v.txt", "--out", "o.ply", "--width", "8", "--height", "8", "--fovy", "60"],
    ["--no-such-option"],
    ["--iters"],
], ids=["none", "incomplete", "empty-frame", "bad-number", "no-iters", "unknown", "no-value"])
def test_cli_usage_errors(args):
    r = subprocess.run([TRAIN] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "usage: gsrt_train" in r.stderr
