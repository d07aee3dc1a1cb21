"""gsrt_normal_noise's generator on the host (gsrt_debug_philox) against a numpy Philox4x32-10 (tests/philox_ref.py), which
is first held to Random123's published known-answer vectors; the declarations of the training session's entry points;
gsrt_lr_expon against 3DGS's formula in float64. No device."""
import ctypes
import os
import re

import numpy as np
import pytest

import gsrt
import philox_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["gsrt_normal_noise", "gsrt_normal_noise_async", "gsrt_model_remap", "gsrt_model_remap_async", "gsrt_ply_write",
       "gsrt_lr_expon", "gsrt_trainer_create", "gsrt_trainer_destroy", "gsrt_trainer_step", "gsrt_trainer_densify",
       "gsrt_trainer_opacity_reset", "gsrt_trainer_rebuild_bvh", "gsrt_trainer_scene", "gsrt_trainer_info",
       "gsrt_trainer_state", "gsrt_trainer_download"]


def test_reference_meets_the_known_answers():
    for ctr, key, want in P.KAT:
        got = P.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert [hex(int(x)) for x in got] == [hex(x) for x in want]
    # vectorised: the three at once
    got = P.philox4x32_10(np.array([k[0] for k in P.KAT], np.uint32), np.array([k[1] for k in P.KAT], np.uint32))
    assert got.tolist() == [list(k[2]) for k in P.KAT]


@pytest.mark.parametrize("seed,stream_id,first,blocks", [
    (0, 0, 0, 1), (1, 0, 0, 257), (0x299f31d0a4093822, 0x13198a2e, 0x85a308d3243f6a88, 5),
    (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF - 2, 6),   # the block counter carries into its high word
    (12345, 7, 65536, 1024),
])
def test_hook_matches_the_reference(seed, stream_id, first, blocks):
    got = gsrt.philox_words(seed, stream_id, first, blocks)
    want = P.words(seed, stream_id, first, blocks)
    assert got.dtype == np.uint32 and got.tobytes() == want.tobytes()


def test_hook_at_the_zero_vector_is_the_published_one():
    assert gsrt.philox_words(0, 0, 0, 1)[0].tolist() == list(P.KAT[0][2])
    assert gsrt.lib.gsrt_debug_philox(0, 0, 0, 1, None) == gsrt.E_ARG
    assert gsrt.lib.gsrt_debug_philox(0, 0, 0, 0, None) == gsrt.OK


def test_new_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "gsrt.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(gsrt_[a-z0-9_]+)\s*\(", text))
    hooks = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsrt_test.h")).read(), flags=re.S)
    assert "gsrt_debug_philox" in set(re.findall(r"\b(gsrt_[a-z0-9_]+)\s*\(", hooks)) and "gsrt_debug_philox" not in declared
    for name in NEW:
        assert name in declared, name
        assert name in gsrt.EXPORTS and hasattr(gsrt.lib, name), name
    assert "gsrt_debug_philox" in gsrt.EXPORTS
    assert len(set(gsrt.EXPORTS)) == len(gsrt.EXPORTS)
    assert gsrt.lib.gsrt_abi_version() == 2


def lr_ref(lr_init, lr_final, step, max_steps, delay_mult, delay_steps):
    """3DGS's get_expon_lr_func, float64"""
    if lr_init == 0.0 and lr_final == 0.0:
        return 0.0
    delay = 1.0
    if delay_steps > 0:
        delay = delay_mult + (1 - delay_mult) * np.sin(0.5 * np.pi * np.clip(step / delay_steps, 0, 1))
    t = np.clip(step / max_steps, 0, 1)
    return delay * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)


@pytest.mark.parametrize("delay_mult,delay_steps", [(1.0, 0), (0.01, 0), (0.01, 1000)])
def test_lr_expon(delay_mult, delay_steps):
    init, final, max_steps = np.float32(1.6e-4), np.float32(1.6e-6), 30000
    for step in (0, 1, 500, 1000, 15000, 29999, 30000, 30001, 4000000000):
        got = gsrt.lr_expon(init, final, step, max_steps, delay_mult, delay_steps)
        want = lr_ref(float(init), float(final), step, max_steps, float(np.float32(delay_mult)), delay_steps)
        # computed in double and rounded once: half an ulp of the float32 result, plus libm's last-bit freedom in double
        assert abs(got - want) <= 2.0 ** -24 * abs(want) * (1 + 1e-6), (step, got, want)
    if delay_steps == 0:
        assert gsrt.lr_expon(init, final, 0, max_steps, delay_mult, 0) == float(init)
        assert gsrt.lr_expon(init, final, max_steps, max_steps, delay_mult, 0) == pytest.approx(float(final), rel=1e-6)
        mid = gsrt.lr_expon(init, final, max_steps // 2, max_steps, delay_mult, 0)
        assert mid == pytest.approx(np.sqrt(float(init) * float(final)), rel=1e-6)   # log-linear: the geometric mean
    else:
        assert gsrt.lr_expon(init, final, 0, max_steps, delay_mult, delay_steps) == pytest.approx(0.01 * float(init), rel=1e-6)


def test_lr_expon_refusals():
    assert gsrt.lr_expon(0.0, 0.0, 5, 10) == 0.0
    out = ctypes.c_float()
    ref = ctypes.byref(out)
    assert gsrt.lib.gsrt_lr_expon(1e-3, 1e-4, 1.0, 0, 10, 0, None) == gsrt.E_ARG
    assert gsrt.lib.gsrt_lr_expon(1e-3, 1e-4, 1.0, 0, 0, 0, ref) == gsrt.E_ARG
    assert gsrt.lib.gsrt_lr_expon(-1e-3, 1e-4, 1.0, 0, 10, 0, ref) == gsrt.E_ARG
    assert gsrt.lib.gsrt_lr_expon(float("nan"), 1e-4, 1.0, 0, 10, 0, ref) == gsrt.E_ARG
    assert gsrt.lib.gsrt_lr_expon(1e-3, 0.0, 1.0, 0, 10, 0, ref) == gsrt.E_ARG
    assert gsrt.lib.gsrt_lr_expon(1e-3, 1e-4, float("nan"), 0, 10, 0, ref) == gsrt.E_ARG
