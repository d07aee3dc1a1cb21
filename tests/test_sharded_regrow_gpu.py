"""The sharded frame's buffers regrown in sequence on one context (gsrt_render_sharded_async, gsrt_comm.cpp).

The loopback tests of test_render_gpu.py pin the exchange path at fixed frame sizes. Here one context renders rank 0's
share of a 4-rank frame (GSRT_DEBUG_RANK_OF=4: the gather buffers, the stand-in receive, the unpack and the code
framebuffer are all in play) over frame sizes that grow, in three frame types that take turns in the same two packed
buffers, with earlier frames still in flight when a buffer is freed and allocated again.
"""
import numpy as np
import pytest

import gsrt

pytestmark = pytest.mark.gpu

N = 4  # ranks of the emulated job; this GPU renders rank 0's share
SIZES = [(64, 48), (160, 96), (320, 200)]
SPP = {"rgba": 4, "d4": 4, "d128": 128}  # d4, d128: FLAG_OUT_DUMP8; 128 spp is 128 passes (the running sums, d_accum)
D8 = gsrt.MODE_COR | gsrt.FLAG_OUT_DUMP8

# (size, type, blocking). Sharded frames 0, 8, 16, ... are profile frames (bands not pinned): frame 0 allocates the
# profile buffers, frames 8 and 24 are the first of a type at a larger size with more tile rows (d_tcost and d_prof
# regrow), frames 16 and 32 repeat the geometry of the profile frame before them (they may adopt the bands cut from its
# profile) and are checked. Frames 4, 5, 7, 12, 13, 17 and 18 grow the other buffers between profile frames, frames 6 and
# 14 go back to a smaller size. Every blocking frame follows two or more frames that were only queued.
FRAMES = [
    (0, "rgba", False), (0, "d4", False), (0, "d128", True), (0, "rgba", False),
    (1, "rgba", False), (1, "d4", True), (0, "d128", False), (1, "d128", False),
    (1, "rgba", False), (1, "d4", False), (1, "rgba", True), (1, "d128", False),
    (2, "d4", False), (2, "d128", True), (1, "d4", False), (1, "rgba", False),
    (1, "rgba", True), (2, "rgba", False), (2, "d128", False), (2, "d4", True),
    (2, "d128", False), (1, "d4", False), (2, "rgba", True), (2, "d4", False),
    (2, "rgba", False), (2, "d4", False), (2, "d128", True), (2, "rgba", False),
    (0, "d4", False), (2, "d128", True), (2, "d4", False), (2, "rgba", False),
    (2, "rgba", True), (2, "d128", False), (1, "rgba", False), (2, "d4", True),
]


def _check_rgba(cx, u, single, fb, where):
    used = cx.last_bands()
    pl = gsrt.tile_plan(u, gsrt.MODE_COR, N, 0)
    assert used.size == N + 1 and used[0] == 0 and used[-1] == pl["tiles_y"], where
    want = gsrt.tile_pack(u, single, N, 0, bands=used).reshape(-1)
    m = pl["tiles_x"] * int(used[1]) * pl["tile_w"] * pl["tile_h"] * 4
    assert cx.debug_gathered(m).tobytes() == want[:m].tobytes(), where
    # the root unpacks its own block and the stand-in (zero) blocks of the others into the framebuffer
    blocks = np.zeros((N, want.size), np.float32)
    blocks[0] = want
    assert fb.tobytes() == gsrt.tile_unpack(u, blocks.reshape(-1), N, bands=used).tobytes(), where
    return used


def _check_dump8(cx, u, single, where):
    """as test_render_gpu.py::test_dump8_root_share: the block's code words are the host mirror's word for word on the
    rank's tiles, its escape list holds the same entries (in arrival order on the device), and gsrt_dump8_read gives
    the single-device frame's codes and escapes on rank 0's rows, code 0 elsewhere"""
    w, h = int(u["width"][0]), int(u["height"][0])
    used = cx.last_bands()
    pl = gsrt.tile_plan(u, D8, N, 0)
    assert used.size == N + 1 and used[0] == 0 and used[-1] == pl["tiles_y"], where
    L = gsrt.dump8_layout(u, N, used, D8)
    dev = cx.debug_gathered(L["block"] * N).view(np.uint32).reshape(N, L["block"])
    host = gsrt.tile_pack_dump8(u, single, N, 0, D8, bands=used)
    n_used = int(used[1]) * pl["tiles_x"] * pl["tile_w"] * pl["tile_h"]
    assert dev[0, :n_used].tobytes() == host[:n_used].tobytes() and not dev[1:].any(), where
    ne = int(host[L["codes"]])
    assert int(dev[0, L["codes"]]) == ne, where
    de = dev[0, L["codes"] + 4:L["codes"] + 4 + 4 * ne].reshape(ne, 4)
    he = host[L["codes"] + 4:L["codes"] + 4 + 4 * ne].reshape(ne, 4)
    assert de[np.argsort(de[:, 0])].tobytes() == he.tobytes(), where
    codes, esc = cx.dump8_read(w, h)
    wc, we = gsrt.dump8_encode(single)
    y1 = min(h, int(used[1]) * pl["tile_h"])
    assert codes[:y1].tobytes() == wc[:y1].tobytes() and not codes[y1:].any(), where
    assert esc.tobytes() == we[we["pixel"] < y1 * w].tobytes(), where
    return used, ne


def test_sharded_buffers_regrow_in_flight(monkeypatch):
    """FRAMES on one context: after every blocking frame rank 0's gathered block equals the host pack of the
    single-device frame of the same camera under the bands that frame was rendered with (gsrt_last_bands), the root's
    framebuffer or gsrt_dump8_read equals that frame on rank 0's rows. Equality only."""
    c, rr, s_, o, sh = gsrt.synth_cloud(gsrt.SYNTH_COR, 2000, 61, True)
    with gsrt.Context(0) as cx:
        sc = gsrt.Scene.from_model(cx, c, rr, s_, o, 20.0 * sh)  # some pixels pass 1022/255: escapes
        sc.build_bvh()
        ubos = {(i, spp): gsrt.camera_from_modelview(gsrt.lookat((0.1, 0.0, 0.3), (0, 0, -1)), 60.0, w, h, 1.0, spp, 16)
                for i, (w, h) in enumerate(SIZES) for spp in (4, 128)}
        singles = {k: sc.render(u, gsrt.MODE_COR)[0] for k, u in ubos.items()}  # computed once, never written again
        monkeypatch.setenv("GSRT_DEBUG_RANK_OF", str(N))
        cx.comm_init_loopback()
        seen, escapes, checked = set(), 0, 0
        for f, (size, kind, blocking) in enumerate(FRAMES):
            key = (size, SPP[kind])
            u, mode = ubos[key], (gsrt.MODE_COR if kind == "rgba" else D8)
            where = f"frame {f}: {SIZES[size]} {kind}"
            if not blocking:
                sc.render_sharded_async(u, mode)
                continue
            fb = sc.render_sharded(u, mode)
            if kind == "rgba":
                used = _check_rgba(cx, u, singles[key], fb, where)
            else:
                assert fb is None
                used, ne = _check_dump8(cx, u, singles[key], where)
                escapes += ne
            even = gsrt.tile_bands(u, N, None, mode)
            seen.add((f, tuple(int(v) for v in used) == tuple(int(v) for v in even)))
            checked += 1
        print(f"{checked} frames checked, {escapes} escapes in rank 0's dump8 blocks")
        assert checked == sum(1 for fr in FRAMES if fr[2])
        assert escapes > 0  # the escape lists are exercised
        # frames 16 and 32 render under bands cut from the profiles of frames 8 and 24 (from rank 0's rows alone: its
        # band shrinks), every other checked frame under the even bands of its geometry
        assert {f for f, is_even in seen if not is_even} == {16, 32}
