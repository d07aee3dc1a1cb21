"""Host side of adaptive density control (gsrt_density_stats_add, gsrt_densify_count, gsrt_densify, gsrt_scene_from_model
with device sources): the header's declarations, the export list, NULL handles and the Python names. No device needed."""
import ctypes
import inspect
import os
import re

import gsrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gsrt.h")).read()
ENTRY_POINTS = ["gsrt_density_stats_add", "gsrt_density_stats_add_async", "gsrt_densify_count", "gsrt_densify",
                "gsrt_densify_async"]


def test_header_and_exports():
    for name in ENTRY_POINTS:
        assert re.search(r"gsrt_status\s+" + name + r"\s*\(", HEADER), name
    for struct, fields in (("gsrt_model_arrays", ["center", "rot_rxyz", "scale", "opacity", "sh", "features",
                                                   "feature_channels"]),
                           ("gsrt_densify_params", ["grad_threshold", "split_scale", "min_opacity", "max_scale", "shrink",
                                                    r"reserved\[3\]"])):
        m = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", HEADER, flags=re.S)
        assert m, struct
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        assert [re.search(r"(\w+(\[3\])?)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()] == \
            [f.replace("\\", "") for f in fields]
    assert re.search(r"#define GSRT_ABI_VERSION 2\b", HEADER)
    assert gsrt.lib.gsrt_abi_version() == 2  # additions only
    assert set(ENTRY_POINTS) <= set(gsrt.EXPORTS)
    assert [f[0] for f in gsrt.ModelArrays._fields_] == ["center", "rot_rxyz", "scale", "opacity", "sh", "features",
                                                         "feature_channels"]
    assert ctypes.sizeof(gsrt.ModelArrays) == 56 and ctypes.sizeof(gsrt.DensifyParams) == 32
    p = gsrt.densify_params(0.0002, 0.01, 0.005)
    assert (p.max_scale, list(p.reserved)) == (0.0, [0, 0, 0]) and abs(p.shrink - 1.6) < 1e-6


def test_null_handles():
    L = gsrt.lib
    assert L.gsrt_density_stats_add(None, 1, 4, 4, None, None) == gsrt.E_ARG
    assert L.gsrt_density_stats_add_async(None, 1, 4, 4, None, None) == gsrt.E_ARG
    assert L.gsrt_densify_count(None, 0, None, None, None, None, None) == gsrt.E_ARG
    assert L.gsrt_densify(None, None, 0, None, None, None, None, None, 0, None) == gsrt.E_ARG
    assert L.gsrt_densify_async(None, None, 0, None, None, None, None, None, 0, None) == gsrt.E_ARG


def test_python_names():
    for name in ("density_stats_add", "densify_count", "densify", "densify_params"):
        assert callable(getattr(gsrt, name)), name
    assert callable(gsrt.Scene.from_model_device)
    auto = open(os.path.join(os.path.dirname(gsrt.__file__), "autograd.py")).read()
    for text in ("def densify(", "def remap_state(", "density_stats=None"):
        assert text in auto
    from gsrt import autograd

    assert "density_stats" in inspect.signature(autograd.render_model).parameters
    assert inspect.signature(autograd.render_model).parameters["density_stats"].default is None
    for step in ("render_model(", "densify(", "remap_state(", "from_model_device(", "build_bvh()", "torch.zeros((n, 2)"):
        assert step in autograd.densify.__doc__, step  # the docstring shows the whole loop
