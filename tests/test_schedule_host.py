"""3DGS's schedule without a device: the entry points of the SH degree ramp-up and the screen-size prune exist in the
library and the header, their ctypes signatures are set, gsrt_train lists both flags, and the refusals that need no device."""
import ctypes
import os
import re
import subprocess

import gsrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gsrt.h")).read()
TRAIN = os.path.join(ROOT, "3dgs-raytrace_amd", "bin", "gsrt_train")
P, U32, F32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float, ctypes.c_uint64
PP = ctypes.POINTER(ctypes.c_void_p)
ENTRY_POINTS = {
    "gsrt_view_stats_add": [P, P, P, P, P],
    "gsrt_view_stats_add_async": [P, P, P, P, P],
    "gsrt_densify_screen": [P, P, U32, P, P, P, P, F32, P, P, U32, P],
    "gsrt_densify_screen_async": [P, P, U32, P, P, P, P, F32, P, P, U32, P],
    "gsrt_densify_screen_count": [P, U32, P, P, P, P, P, F32, P],
    "gsrt_model_step_degree": [P, U32, P, P, P, P, P, U32, P, P, P, P],
    "gsrt_model_step_degree_async": [P, U32, P, P, P, P, P, U32, P, P, P, P],
    "gsrt_trainer_densify_screen": [P, P, F32, U64, P],
    "gsrt_trainer_set_sh_degree": [P, U32],
    "gsrt_trainer_sh_degree": [P, P],
    "gsrt_trainer_radii": [P, PP],
}


def test_symbols_and_signatures():
    assert re.search(r"#define\s+GSRT_ABI_VERSION\s+2\b", HEADER) and gsrt.lib.gsrt_abi_version() == 2
    for name, args in ENTRY_POINTS.items():
        assert re.search(r"gsrt_status\s+" + name + r"\s*\(", HEADER), name
        assert name in gsrt.EXPORTS, name
        fn = getattr(gsrt.lib, name)
        assert fn.argtypes == args and fn.restype is ctypes.c_int, name
    # the two entries left the "Not provided" lists
    assert "SH degree ramp-up;" not in HEADER and "screen-radius pruning" not in HEADER
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "gsrt_view_stats_add" in readme and "gsrt_model_step_degree" in readme
    assert "--sh-degree-every" in readme and "--max-screen-radius" in readme
    # the header states the arithmetic of the radius and what the frames still do
    for text in ("mid  = 0.5f * (v00 + v11)", "disc = fmaf(mid, mid, -det)", "lam  = mid + sqrtf(fmaxf(0.1f, disc))",
                 "r    = ceilf(3.0f * sqrtf(lam))", "a NaN r stores nothing", "3 (sh_degree + 1)^2",
                 "still evaluate all 16 coefficients", "radii[g] > max_screen_radius"):
        assert text in HEADER, text


def test_python_keywords():
    import inspect

    for fn, names in ((gsrt.densify, ("radii", "max_screen_radius")), (gsrt.densify_count, ("radii", "max_screen_radius")),
                      (gsrt.model_step, ("sh_degree",)), (gsrt.Trainer.densify, ("max_screen_radius",)),
                      (gsrt.view_stats_add, ("radii",)), (gsrt.Scene.view_stats_add, ("radii",))):
        have = inspect.signature(fn).parameters
        assert all(k in have for k in names), fn
    assert inspect.signature(gsrt.model_step).parameters["sh_degree"].default == 3
    assert inspect.signature(gsrt.Trainer.densify).parameters["max_screen_radius"].default == 0.0
    assert isinstance(gsrt.Trainer.sh_degree, property) and callable(gsrt.Trainer.radii)


def test_null_handles_are_refused():
    L = gsrt.lib
    u, h = ctypes.c_uint32(7), ctypes.c_void_p()
    model, grads = gsrt.ModelArrays(), gsrt.ModelGrads()
    adam, dens = gsrt.adam_params(), gsrt.densify_params(1.0, 1.0, 0.0)
    ubo = gsrt.camera_from_modelview(gsrt.translate(0, 0, -2), 60.0, 8, 8)
    assert L.gsrt_view_stats_add(None, gsrt._p(ubo), None, None, None) == gsrt.E_ARG
    assert L.gsrt_view_stats_add_async(None, gsrt._p(ubo), None, None, None) == gsrt.E_ARG
    m = ctypes.byref(model)
    assert L.gsrt_densify_screen(None, m, 0, None, None, ctypes.byref(dens), None, 20.0, m, None, 0, ctypes.byref(u)) == gsrt.E_ARG
    assert L.gsrt_densify_screen_async(None, m, 0, None, None, ctypes.byref(dens), None, 20.0, m, None, 0, None) == gsrt.E_ARG
    assert L.gsrt_densify_screen_count(None, 0, None, None, None, ctypes.byref(dens), None, 20.0, ctypes.byref(u)) == gsrt.E_ARG
    assert u.value == 7
    for fn in (L.gsrt_model_step_degree, L.gsrt_model_step_degree_async):
        assert fn(None, 0, m, m, m, ctypes.byref(grads), ctypes.byref(adam), 0, None, None, None, None) == gsrt.E_ARG
    assert L.gsrt_trainer_densify_screen(None, ctypes.byref(dens), 20.0, 0, ctypes.byref(u)) == gsrt.E_ARG and u.value == 7
    assert L.gsrt_trainer_set_sh_degree(None, 0) == gsrt.E_ARG
    assert L.gsrt_trainer_sh_degree(None, ctypes.byref(u)) == gsrt.E_ARG and u.value == 7
    assert L.gsrt_trainer_radii(None, ctypes.byref(h)) == gsrt.E_ARG and not h.value


def test_cli_help_lists_both_flags():
    r = subprocess.run([TRAIN, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "usage: gsrt_train" in text
    assert "--sh-degree-every N" in text and "--max-screen-radius R" in text
    bad = subprocess.run([TRAIN, "--max-screen-radius", "-1", "--ply", "a.ply", "--views", "v", "--out", "o", "--width", "8",
                          "--height", "8", "--fovy", "60", "--iters", "1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--max-screen-radius" in bad.stderr
