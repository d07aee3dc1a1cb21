"""Which whole frames the library refuses, and with which words (gsrt_debug_frame_refusal, the function every whole-frame
entry point asks): equal to tests/golden/frame_refusals.npz over the whole product of modes, callers and scene facts. The
golden holds what the hand-written refusal blocks of commit e1f9c6a answered (tests/golden/gen_frame_refusals.cpp carries
their text); run as a script, this module packs that program's output into the golden. No device needed."""
import ctypes
import itertools
import os
import sys

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_refusals.npz")
CALLERS = (0, 1, 2, 3)  # GradKind: none, feature, sh, opacity
PASSES = ((1, 1), (0, 1), (1, 0))  # (samples, bvh_built)


def frame_refusal(mode, caller=0, samples=1, bvh_built=1, ntri=0, features=0, sh=0):
    """(status, gsrt_last_error text) a whole frame of `mode` gets from its entry point: caller 0 is no gradient call, 1
    feature_grad, 2 sh_grad, 3 opacity_grad; the rest are the scene's facts"""
    import gsrt

    msg = ctypes.create_string_buffer(256)
    s = gsrt.lib.gsrt_debug_frame_refusal(mode, caller, samples, bvh_built, ntri, features, sh, msg, len(msg))
    return s, msg.value.decode()


def cases():
    """(mode, caller, samples, bvh_built, ntri, features, sh) in the generator's order"""
    for (samples, built), low, bits, caller, ntri, feat, sh in itertools.product(
            PASSES, (0, 1, 2), range(512), CALLERS, (0, 1), (0, 1), (0, 1)):
        yield low | bits << 8, caller, samples, built, ntri, feat, sh


def test_refusals_equal_the_parents():
    import gsrt

    g = np.load(GOLDEN)
    status, message, index = g["status"], [str(m) for m in g["message"]], g["index"]
    assert index.size == 3 * 3 * 512 * 4 * 8 and len(message) == status.size == int(index.max()) + 1
    assert (gsrt.MODE_REF, gsrt.MODE_COR, gsrt.FLAG_LUT, gsrt.FLAG_OPACITY_GRAD) == (0, 1, 0x100, 0x8000)
    wrong = []
    n = 0
    for n, (case, want) in enumerate(zip(cases(), index), 1):
        got = frame_refusal(*case)
        if got != (int(status[want]), message[want]):
            wrong.append((case, got, (int(status[want]), message[want])))
    assert n == index.size
    assert not wrong, (len(wrong), wrong[:5])


def test_ok_has_no_message_and_arguments_are_checked():
    import gsrt

    assert frame_refusal(gsrt.MODE_COR, 0) == (gsrt.OK, "")
    assert frame_refusal(gsrt.MODE_COR | gsrt.FLAG_SH_GRAD, 2, sh=1) == (gsrt.OK, "")
    assert gsrt.lib.gsrt_debug_frame_refusal(gsrt.MODE_COR, 4, 1, 1, 0, 0, 0, None, 0) == gsrt.E_ARG  # no such caller
    # a short buffer truncates the message and keeps it terminated
    buf = ctypes.create_string_buffer(b"x" * 16, 16)
    assert gsrt.lib.gsrt_debug_frame_refusal(gsrt.MODE_COR | 0x10000, 0, 1, 1, 0, 0, 0, buf, 4) == gsrt.E_ARG
    assert buf.raw[:5] == b"bad\0x"


if __name__ == "__main__":  # gen_frame_refusals | python tests/test_frame_refusal_host.py
    head, _, tail = sys.stdin.read().partition("\n\n")
    answers = [line.split("\t", 1) for line in head.split("\n")]
    idx = np.array(tail.split(), np.uint16)
    assert idx.size == sum(1 for _ in cases()) and int(idx.max()) == len(answers) - 1
    np.savez_compressed(GOLDEN, status=np.array([int(s) for s, _ in answers], np.int32),
                        message=np.array([m for _, m in answers]), index=idx)
    print(f"{GOLDEN}: {idx.size} cases, {len(answers)} distinct answers")
