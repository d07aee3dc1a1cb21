"""The bits of everything that runs the COR projection chain, for comparing two builds of the library.

  GSRT_LIB_PATH=<one libgsrt.so> python3 profiles/project_chain/bits.py [--out FILE] [--rows FILE.npz]

Run once per library, each run its own process; every line is {"output": name, "sha256": hash} for fixed seeded inputs, and
the two runs' lines must be equal. Nothing here is compared against a reference: that is the suite's work.

The chain kernels (gsrt_splat_grad_to_model, its depth form, gsrt_pose_grad plain and depth) at n = 1, 255, 256, 257, 2049
and 2 * 2048 + 1 (the 256-lane and kPoseChunk seams) on tests/pose_cases.py's synthetic model, in which every sixth Gaussian
stands behind the camera, with, from n = 3 on, Gaussian 1 given an indefinite cov3d (det < 0), Gaussian 2 a cov3d of 1e30
(V overflows: det is not finite), and every Gaussian with index % 6 == 3 (valid) an all-+0 row. n = 2049 runs a second time
under a non-affine view and a general projection. The model chain's outputs are hashed after a writing call and again after
an accumulating call on top of it.

The forward: the smallest frame of the geometry tests' case table (tests/test_grad_f64.py's CASES[-1]), as a COR frame, a
COR depth frame and the splat rows of a seeded upstream gradient, once through the fused prep kernel (k_prep_cor, the
pipelined path) and once through k_project (GSRT_DEBUG_NO_FRONTIER=1), and the COR frame of the counting pass
(GSRT_FLAG_STATS, the blocking path, k_project). The splat rows are sums of float atomics, whose order is not fixed: two
takes by one library differ in their last bits, so their hashes say nothing. They are taken three times and written to
--rows FILE (.npz) instead; compare.py sets the difference between the libraries beside the difference between two takes
of one.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("3dgs-raytrace_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
import gsrt  # noqa: E402
import pose_cases as PC  # noqa: E402
import test_grad_f64 as S  # noqa: E402

SIZES = [1, 255, 256, 257, 2049, 2 * 2048 + 1]
LINES = []
ROWS = {}


def emit(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    LINES.append(json.dumps({"output": name, "sha256": h.hexdigest()}))
    print(LINES[-1], flush=True)


def model(n, ubo):
    params, aabbs, rows, _ = PC.synthetic(n, 900 + n, ubo)
    if n >= 3:
        params[1, 4:10] = (100.0, 0.0, 0.0, -100.0, 0.0, 0.01)
        params[2, 4:10] = (1e30, 0.0, 0.0, 1e30, 0.0, 1e30)
        aabbs[1:3, :3] = params[1:3, :3] - 1.0  # the chain never reads the boxes; the BVH build gets finite ones
        aabbs[1:3, 3:] = params[1:3, :3] + 1.0
    rows[np.arange(n) % 6 == 3] = 0.0
    return params, aabbs, rows


def chain(ctx, n, ubo, label):
    params, aabbs, rows = model(n, ubo)
    sc = gsrt.Scene.from_params(ctx, params, aabbs)
    try:
        sc.build_bvh()
        d_rows = torch.from_numpy(rows).to("cuda:0")
        for depth in (False, True):
            form = "depth" if depth else "plain"
            d_c = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda:0")
            d_v = torch.full((n, 6), 7.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            sc.model_grad_async(ubo, d_rows.data_ptr(), d_c.data_ptr(), d_v.data_ptr(), depth=depth)
            ctx.synchronize()
            emit(f"model_grad {label} n={n} {form}", d_c.cpu().numpy(), d_v.cpu().numpy())
            sc.model_grad_async(ubo, d_rows.data_ptr(), d_c.data_ptr(), d_v.data_ptr(), accumulate=True, depth=depth)
            ctx.synchronize()
            emit(f"model_grad {label} n={n} {form} accumulate", d_c.cpu().numpy(), d_v.cpu().numpy())
            emit(f"pose_grad {label} n={n} {form}", sc.pose_grad(ubo, rows, depth=depth))
    finally:
        sc.close()


def forward(ctx):
    case = S.CASES[-1]
    assert case == min(S.CASES, key=lambda c: c[1] * c[2])
    c, r, s, o, sh = S.scene()
    ubo = S.camera(*case)
    _, w, h, _ = case
    G = S.noise(w * h, 4, 41).reshape(h, w, 4)
    sc = gsrt.Scene.from_model(ctx, c, r, s, o, sh)
    try:
        sc.build_bvh()
        emit("frame k_project stats", sc.render(ubo, gsrt.MODE_COR | gsrt.FLAG_STATS)[0])
        for path, env in (("k_prep_cor", "0"), ("k_project", "1")):
            os.environ["GSRT_DEBUG_NO_FRONTIER"] = env  # read per frame
            emit(f"frame {path}", sc.render(ubo)[0])
            emit(f"depth frame {path}", *sc.render_depth(ubo))
            ROWS[path] = np.stack([sc.splat_grad(ubo, G) for _ in range(3)])
        os.environ["GSRT_DEBUG_NO_FRONTIER"] = "0"
    finally:
        sc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rows", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bits: no GPU")
    with gsrt.Context(0) as ctx:
        for n in SIZES:
            chain(ctx, n, PC.camera(), "affine")
        chain(ctx, 2049, PC.nonaffine_camera(), "non-affine")
        forward(ctx)
    if a.rows:
        np.savez(a.rows, **ROWS)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps({"library": os.environ.get("GSRT_LIB_PATH", "libgsrt.so"), "outputs": len(LINES)}) + "\n")
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
