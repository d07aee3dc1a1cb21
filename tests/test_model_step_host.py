"""Host side of the optimiser step (gsrt_adam_scalars, gsrt_model_step, gsrt_model_activate, gsrt_model_deactivate,
gsrt_model_opacity_reset): the header's declarations and the export list, every refusal that can be reached without a
context, the structs' sizes and offsets as a C compiler lays them out against the ctypes mirrors, the Python names, and
the documents. No device needed."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import gsrt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gsrt.h")).read()
ENTRY_POINTS = ["gsrt_adam_scalars", "gsrt_model_step", "gsrt_model_step_async", "gsrt_model_activate",
                "gsrt_model_activate_async", "gsrt_model_deactivate", "gsrt_model_deactivate_async",
                "gsrt_model_opacity_reset", "gsrt_model_opacity_reset_async"]


def test_header_and_exports():
    for name in ENTRY_POINTS:
        assert re.search(r"gsrt_status\s+" + name + r"\s*\(", HEADER), name
        assert hasattr(gsrt.lib, name), name
    assert set(ENTRY_POINTS) <= set(gsrt.EXPORTS)
    assert re.search(r"#define GSRT_ABI_VERSION 2\b", HEADER)
    assert gsrt.lib.gsrt_abi_version() == 2  # additions only
    assert HEADER.index("gsrt_image_loss_window(") < HEADER.index("gsrt_adam_scalars(")
    section = HEADER[HEADER.index("---- the optimiser step"):HEADER.index("gsrt_status gsrt_model_opacity_reset_async")]
    for text in ("Everything is float32", "no fused multiply-add", "nq == 0", "expf(-t)", "(ss * m') / (sqrtf(v') / c2 + eps)",
                 "GSRT_ADAM_SPARSE", "keep their bits", "gsrt_synchronize before handing params_out", "on other streams",
                 "bit for bit, what gsrt_scene_from_model writes", "a NaN logit stays a NaN"):
        assert text in section, text
    assert re.search(r"#define GSRT_ADAM_SPARSE 1u\b", HEADER) and gsrt.ADAM_SPARSE == 1


def good():
    return gsrt.adam_params(step=1)


def scalars_status(adam):
    out = np.zeros(gsrt.ADAM_SCALARS, np.float32)
    return gsrt.lib.gsrt_adam_scalars(ctypes.byref(adam), out.ctypes.data_as(ctypes.c_void_p)), out


def test_adam_scalars_accepts_and_refuses():
    st, out = scalars_status(good())
    assert st == gsrt.OK and out[:3].all()
    assert gsrt.lib.gsrt_adam_scalars(None, out.ctypes.data_as(ctypes.c_void_p)) == gsrt.E_ARG
    assert gsrt.lib.gsrt_adam_scalars(ctypes.byref(good()), None) == gsrt.E_ARG
    bad = []
    for field, values in (("step", [0]), ("beta1", [1.0, -0.1, 1.5, float("nan")]), ("beta2", [1.0, -0.1, float("nan")]),
                          ("eps", [0.0, -1e-8, float("nan")]), ("flags", [2, 0x80000001])):
        for value in values:
            a = good()
            setattr(a, field, value)
            bad.append((field, value, a))
    for group in ("center", "rot", "scale", "opacity", "sh_dc", "sh_rest", "features"):
        for value in (-1e-3, float("nan")):
            a = good()
            setattr(a, "lr_" + group, value)
            bad.append(("lr_" + group, value, a))
    for word in range(4):
        a = good()
        a.reserved[word] = 1
        bad.append(("reserved", word, a))
    for field, value, a in bad:
        out = np.full(gsrt.ADAM_SCALARS, 7.0, np.float32)
        assert gsrt.lib.gsrt_adam_scalars(ctypes.byref(a), out.ctypes.data_as(ctypes.c_void_p)) == gsrt.E_ARG, (field, value)
        assert (out == 7.0).all(), (field, value)  # nothing written
        with pytest.raises(gsrt.GsrtError):
            gsrt.adam_scalars(a)
    # the edges that are allowed: beta = 0, lr = 0 (a frozen group), a lone sparse flag, the largest step
    a = gsrt.adam_params(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1e-30, 0xFFFFFFFF, True)
    st, out = scalars_status(a)
    assert st == gsrt.OK and out.tolist() == [1.0, 1.0, 1.0] + [0.0] * 7


def test_null_handles():
    L = gsrt.lib
    arrays, grads, adam = gsrt.ModelArrays(), gsrt.ModelGrads(), good()
    r = ctypes.byref
    assert L.gsrt_model_step(None, 0, r(arrays), r(arrays), r(arrays), r(grads), r(adam), None, None, None, None) == gsrt.E_ARG
    assert L.gsrt_model_step_async(None, 0, r(arrays), r(arrays), r(arrays), r(grads), r(adam), None, None, None, None) == gsrt.E_ARG
    assert L.gsrt_model_activate(None, 0, r(arrays), None, None, None) == gsrt.E_ARG
    assert L.gsrt_model_activate_async(None, 0, r(arrays), None, None, None) == gsrt.E_ARG
    assert L.gsrt_model_deactivate(None, 0, r(arrays), r(arrays)) == gsrt.E_ARG
    assert L.gsrt_model_deactivate_async(None, 0, r(arrays), r(arrays)) == gsrt.E_ARG
    assert L.gsrt_model_opacity_reset(None, 0, None, None, None, 0.01) == gsrt.E_ARG
    assert L.gsrt_model_opacity_reset_async(None, 0, None, None, None, 0.01) == gsrt.E_ARG


C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "gsrt.h"
#define F(T, f) printf(#T "." #f " %zu\n", offsetof(T, f))
int main(void) {
    printf("gsrt_adam_params %zu\n", sizeof(gsrt_adam_params));
    printf("gsrt_model_grads %zu\n", sizeof(gsrt_model_grads));
    printf("gsrt_model_arrays %zu\n", sizeof(gsrt_model_arrays));
    F(gsrt_adam_params, lr_center); F(gsrt_adam_params, lr_rot); F(gsrt_adam_params, lr_scale);
    F(gsrt_adam_params, lr_opacity); F(gsrt_adam_params, lr_sh_dc); F(gsrt_adam_params, lr_sh_rest);
    F(gsrt_adam_params, lr_features); F(gsrt_adam_params, beta1); F(gsrt_adam_params, beta2); F(gsrt_adam_params, eps);
    F(gsrt_adam_params, step); F(gsrt_adam_params, flags); F(gsrt_adam_params, reserved);
    F(gsrt_model_grads, center); F(gsrt_model_grads, cov); F(gsrt_model_grads, splat); F(gsrt_model_grads, sh);
    F(gsrt_model_grads, features);
    return 0;
}
"""


def test_struct_layout_against_a_c_compiler(tmp_path):
    """the header compiled as C: sizes and offsets are those of the ctypes mirrors"""
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(C_PROBE)
    subprocess.run(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                   check=True)
    lines = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                check=True).stdout.splitlines())
    mirrors = {"gsrt_adam_params": gsrt.AdamParams, "gsrt_model_grads": gsrt.ModelGrads, "gsrt_model_arrays": gsrt.ModelArrays}
    for name, cls in mirrors.items():
        assert int(lines.pop(name)) == ctypes.sizeof(cls), name
    assert ctypes.sizeof(gsrt.AdamParams) == 64 and ctypes.sizeof(gsrt.ModelGrads) == 40
    assert len(lines) == 18
    for key, offset in lines.items():
        struct, field = key.split(".")
        assert getattr(mirrors[struct], field).offset == int(offset), key
    assert [f for f, _ in gsrt.AdamParams._fields_] == ["lr_center", "lr_rot", "lr_scale", "lr_opacity", "lr_sh_dc",
                                                       "lr_sh_rest", "lr_features", "beta1", "beta2", "eps", "step",
                                                       "flags", "reserved"]


def test_python_names():
    sig = inspect.signature(gsrt.model_step)
    assert list(sig.parameters)[:6] == ["ctx", "raw", "m", "v", "grads", "adam"]
    assert sig.parameters["n"].kind is inspect.Parameter.KEYWORD_ONLY
    for name in ("adam_params", "adam_scalars", "model_step", "model_activate", "model_deactivate", "model_opacity_reset"):
        assert callable(getattr(gsrt, name)), name
    a = gsrt.adam_params()
    assert (a.beta1, a.beta2, a.eps, a.step, a.flags) == (np.float32(0.9), np.float32(0.999), np.float32(1e-15), 1, 0)
    assert gsrt.adam_params(sparse=True).flags == gsrt.ADAM_SPARSE
    from gsrt import autograd

    assert list(inspect.signature(autograd.model_step).parameters)[:6] == ["ctx", "raw", "m", "v", "grads", "adam"]
    doc = autograd.model_step.__doc__
    order = ["scene.render_async(", "gsrt.image_loss(", "scene.splat_grad_async(", "scene.model_grad_async(",
             "scene.sh_grad_async(", "model_step(ctx, raw, m, v", "scene.update(", "scene.refit_bvh()", "scene.set_sh("]
    at = [doc.index(s) for s in order]
    assert at == sorted(at)  # the whole loop, in order
    for s in ("densify(", "remap_state", "model_deactivate", "model_opacity_reset"):
        assert s in doc, s
    assert "torch.optim" not in doc.split("The whole loop")[1].split("\n", 1)[1]


def test_documents():
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"^- \*\*Optimiser step", readme, flags=re.M)
    assert "an opacity reset" not in readme
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in ("k_model_geom", "k_model_rows", "weight decay", "learning-rate schedules", "SH degree ramp-up"):
        assert text in design, text
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in ("gsrt_model_step_async(", "gsrt_model_deactivate(", "gsrt_model_opacity_reset"):
        assert text in integ, text
